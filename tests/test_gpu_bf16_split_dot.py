"""GPU: the split gather-dot of bfloat16 layers (k_split_dot.hip: sd_e1_dot_kernel, the error staged in one binary16 limb).

A bf16 dy times its channel's power-of-two scale is its own hi limb, so leaving out the product with the (zero) lo limb leaves
every accumulator chain of the three-product kernel as it was: the four parameter gradients of a bf16 plan are BIT-IDENTICAL to
those of an fp32 DAU_FLAG_DENSE_SPLIT_F16 plan run on the widened tensors (shapes: the ring's corner cases of
test_gpu_split_gather_dot_ring.py).  Beside that: the fp32 bar against the oracle (which gets the widened values) over unit
counts, region widths and offset ranges; dynamic range across and inside channels (the f16 subnormal tail of a channel);
non-finite values stay in their channel; the hand-over to the exact kernels beyond +-4; the three-product reference build
(libdau_conv_hip_bf16_e2.so of `make tuning`); the layer under torch.autocast."""
import numpy as np
import pytest
import torch

from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, record_margins, variant_capi

pytestmark = pytest.mark.gpu

PARAMS = ("dw", "dmu1", "dmu2", "dsigma")
BAR = "1e-4 rel + 1e-6 max-norm (fp32 bar; bf16 split gather-dot, one-limb error)"


def _capi():
    from dau_conv import _capi
    return _capi


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16)


def _inputs(seed, shape, m, ignore=0):
    """make_inputs with the extreme offsets of the window on the first units; x and dy bf16-rounded (torch tensors)"""
    N, S, F, G, H, W = shape
    x, dy, w, mu1, mu2 = make_inputs(seed, N, S, F, G, H, W, 9, abs(m), ignore=ignore)
    mu1.flat[0] = m; mu2.flat[0] = -m; mu1.flat[1] = -m; mu2.flat[1] = m
    return _bf16(x), _bf16(dy), w, mu1, mu2


def _plan(capi, shape, io, extra=0, k=9, sigma=0.5, ignore=0):
    flags = capi.FLAG_USE_INTERPOLATION | extra | (capi.FLAG_IO_BF16 if io == "bf16" else 0)
    return capi.Plan(*shape, max_kernel_size=k, sigma_hint=sigma, flags=flags, number_units_ignore=ignore)


def _grads(capi, plan, xb, dyb, w, mu1, mu2, sigma=0.5, need=None):
    """the parameter gradients of one backward call; a bf16 plan gets the bf16 tensors, an fp32 plan the widened ones"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    S, G, F = w.shape[1:]
    sg = torch.full((1, S, G, F), float(sigma), device="cuda")
    need = need if need is not None else capi.NEED_DW | capi.NEED_DMU1 | capi.NEED_DMU2 | capi.NEED_DSIGMA
    wide = plan.io_dtype == torch.float32
    xd, dyd = (xb.float() if wide else xb).cuda(), (dyb.float() if wide else dyb).cuda()
    g = plan.backward(xd, dyd, dev(w), dev(mu1), dev(mu2), sg, need_mask=need)
    plan.check_status()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(("dx",) + PARAMS, g) if k in PARAMS and v is not None}


def _same_bits(a, b, name):
    for key in a:
        differ = int((a[key].view(np.uint32) != b[key].view(np.uint32)).sum())
        print("%s/%s: %d of %d values differ" % (name, key, differ, a[key].size))
        assert np.array_equal(a[key], b[key]), "%s/%s: %d values differ" % (name, key, differ)


def _want(xb, dyb, w, mu1, mu2, fs=None, sigma=0.5, **kw):
    x, dy = xb.float().numpy(), dyb.float().numpy()
    if fs is None:
        return orc.backward(x, dy, w, mu1, mu2, sigma, need=PARAMS, **kw)
    return orc.backward(x, dy[:, fs], w[..., fs], mu1[..., fs], mu2[..., fs], sigma, need=PARAMS, **kw)


def _check(name, got, want, keys=PARAMS):
    for key in keys:
        assert_parity(got[key], want[key], name + "/" + key)
    return record_margins("bf16sdot/" + name, {k: got[k] for k in keys}, {k: want[k] for k in keys}, BAR)


# ---- 1. bit-identity with the fp32 plan on the widened input ------------------------------------------------------------------
RING_CASES = [
    ("mid-strip", (8, 256, 256, 4, 27, 27), 3.0, 301),
    ("single-strip", (8, 256, 256, 4, 40, 9), 3.0, 302),
    ("single-row", (16, 256, 256, 4, 3, 40), 3.0, 303),
    ("exact-columns-12", (8, 256, 256, 4, 20, 35), 3.0, 304),
    ("exact-columns-10", (8, 256, 256, 4, 20, 29), 3.0, 304),
    ("ragged", (13, 250, 100, 7, 20, 20), 3.0, 305),
    ("small-ragged", (5, 40, 36, 3, 24, 24), 3.0, 306),
    ("m+3.99", (8, 256, 256, 4, 32, 32), 3.99, 307),
    ("m-3.99", (8, 256, 256, 4, 32, 32), -3.99, 307),
]


@pytest.mark.parametrize("name, shape, m, seed", RING_CASES, ids=[c[0] for c in RING_CASES])
def test_bf16_plan_is_bit_identical_to_the_fp32_plan_on_the_widened_input(name, shape, m, seed):
    capi = _capi()
    case = _inputs(seed, shape, m)
    bf16 = _grads(capi, _plan(capi, shape, "bf16"), *case)                             # the DEFAULT bf16 plan
    fp32 = _grads(capi, _plan(capi, shape, "f32", capi.FLAG_DENSE_SPLIT_F16), *case)
    _same_bits(bf16, fp32, "bf16-vs-fp32/" + name)
    if shape[1] == 256 and shape[2] == 256:
        # the member ran: the exact gather-dot sums in another order
        exact = _grads(capi, _plan(capi, shape, "bf16", capi.FLAG_NO_DENSE_SPLIT), *case)
        assert any(not np.array_equal(exact[k], bf16[k]) for k in PARAMS), name


def test_bf16_plan_bit_identical_without_dsigma_with_the_edge_rule():
    """a need mask without dsigma, the unit_testing edge rule, one ignored unit, sigma 0.8"""
    capi = _capi()
    shape = (2, 12, 20, 4, 32, 32)
    case = _inputs(5, shape, 3.5, ignore=1)
    need = capi.NEED_DW | capi.NEED_DMU1 | capi.NEED_DMU2
    kw = dict(sigma=0.8, ignore=1)
    bf16 = _grads(capi, _plan(capi, shape, "bf16", capi.FLAG_UNIT_TESTING, **kw), *case, sigma=0.8, need=need)
    fp32 = _grads(capi, _plan(capi, shape, "f32", capi.FLAG_UNIT_TESTING | capi.FLAG_DENSE_SPLIT_F16, **kw), *case, sigma=0.8, need=need)
    assert sorted(bf16) == ["dmu1", "dmu2", "dw"]
    _same_bits(bf16, fp32, "bf16-vs-fp32/kinds3")
    _check("kinds3", bf16, _want(*case, sigma=0.8, ignore=1, unit_testing=True), keys=("dw", "dmu1", "dmu2"))


# ---- 2. oracle parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [17, 23], ids=["RW10", "RW12"])
@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 6, 7])
def test_bf16_split_dot_unit_counts(G, W):
    """G = 3, 4, 6, 7: the default plan holds the member; G = 1, 2, 5: forced.  Ragged batch, octet and channel blocks."""
    capi = _capi()
    shape = (3, 20, 36, G, 13, W)
    case = _inputs(70 + G, shape, 3.0)
    forced = capi.FLAG_DENSE_SPLIT_F16 if G in (1, 2, 5) else 0
    got = _grads(capi, _plan(capi, shape, "bf16", forced), *case)
    # (that the member ran: the fp32 member on the widened input gives the same bits, which the exact kernel does not promise)
    _same_bits(got, _grads(capi, _plan(capi, shape, "f32", capi.FLAG_DENSE_SPLIT_F16), *case), "G%d/W%d" % (G, W))
    _check("G%d/W%d" % (G, W), got, _want(*case))


@pytest.mark.parametrize("m", [0.4, 2.0, 3.0, 3.99])
def test_bf16_split_dot_offset_ranges(m):
    capi = _capi()
    shape = (2, 16, 32, 4, 28, 28)
    case = _inputs(81, shape, m)
    _check("m%.2f" % m, _grads(capi, _plan(capi, shape, "bf16"), *case), _want(*case))


# ---- 3. dynamic range ----------------------------------------------------------------------------------------------------------
def test_bf16_split_dot_wide_dynamic_range_across_channels():
    capi = _capi()
    shape = N, S, F, G, H, W = 2, 16, 32, 4, 20, 20
    x, dy, w, mu1, mu2 = make_inputs(9, N, S, F, G, H, W, 9, 3.0)
    x *= (2.0 ** np.linspace(-10, 10, S)).astype(np.float32)[None, :, None, None]
    dy *= (2.0 ** np.linspace(10, -10, F)).astype(np.float32)[None, :, None, None]
    case = (_bf16(x), _bf16(dy), w, mu1, mu2)
    got = _grads(capi, _plan(capi, shape, "bf16"), *case)
    want = _want(*case)
    for f in range(F):                                   # each output channel against its own max-norm
        for key in PARAMS:
            assert_parity(got[key][..., f], want[key][..., f], "bf16sdot/range/%s/f%d" % (key, f))


def test_bf16_split_dot_subnormal_tail_inside_a_channel():
    """a quarter of one dy channel scaled by 2^-30: below 2^-27 of the channel's maximum, so on the f16 subnormal grid"""
    capi = _capi()
    shape = N, S, F, G, H, W = 2, 16, 32, 4, 20, 20
    x, dy, w, mu1, mu2 = make_inputs(10, N, S, F, G, H, W, 9, 3.0)
    tiny = np.random.RandomState(3).rand(N, H, W) < 0.25
    dy[:, 7][tiny] *= np.float32(2.0 ** -30)
    case = (_bf16(x), _bf16(dy), w, mu1, mu2)
    assert float(case[1][:, 7].float().abs().max()) > 1.0 and int(tiny.sum()) > 100
    got = _grads(capi, _plan(capi, shape, "bf16"), *case)
    want = _want(*case)
    for key in PARAMS:
        assert_parity(got[key][..., 7], want[key][..., 7], "bf16sdot/tail/%s/f7" % key)
    _check("tail", got, want)


# ---- 4. non-finite values ------------------------------------------------------------------------------------------------------
def test_bf16_split_dot_non_finite_dy_stays_in_its_output_channel():
    capi = _capi()
    shape = N, S, F, G, H, W = 2, 16, 32, 4, 16, 16
    x, dy, w, mu1, mu2 = make_inputs(11, N, S, F, G, H, W, 9, 3.0)
    dy[1, 5, 3, 3] = np.inf; dy[0, 5, 9, 2] = -np.inf; dy[1, 5, 12, 12] = np.nan
    case = (_bf16(x), _bf16(dy), w, mu1, mu2)
    got = _grads(capi, _plan(capi, shape, "bf16"), *case)
    keep = [f for f in range(F) if f != 5]
    want = _want(*case, fs=keep)
    for key in PARAMS:
        assert_parity(got[key][..., keep], want[key], "bf16sdot/dy-nonfinite/" + key)


def test_bf16_split_dot_inf_in_x_stays_in_its_input_channel():
    capi = _capi()
    shape = N, S, F, G, H, W = 2, 16, 32, 4, 16, 16
    x, dy, w, mu1, mu2 = make_inputs(12, N, S, F, G, H, W, 9, 3.0)
    clean = (_bf16(x), _bf16(dy), w, mu1, mu2)
    x[1, 6, 4, 4] = np.inf
    got = _grads(capi, _plan(capi, shape, "bf16"), _bf16(x), *clean[1:])
    keep = [s for s in range(S) if s != 6]
    want = _want(*clean)                                 # the gradients of a unit depend on its own input channel only
    for key in PARAMS:
        assert_parity(got[key][:, keep], want[key][:, keep], "bf16sdot/x-inf/" + key)


def test_bf16_split_dot_zero_dy_gives_exact_zeros():
    capi = _capi()
    shape = (2, 16, 32, 4, 16, 16)
    xb, dyb, w, mu1, mu2 = _inputs(13, shape, 3.0)
    got = _grads(capi, _plan(capi, shape, "bf16"), xb, torch.zeros_like(dyb), w, mu1, mu2)
    for key in PARAMS:
        assert not got[key].any(), key


# ---- 5. hand-over --------------------------------------------------------------------------------------------------------------
def test_bf16_split_dot_hands_over_beyond_the_window_and_the_hint_decides_nothing():
    capi = _capi()
    shape = (3, 18, 36, 4, 24, 28)
    plan = _plan(capi, shape, "bf16", k=17)
    assert plan.info["bucket_sets"] == 2
    far = _inputs(42, shape, 3.0)
    far[3].flat[5] = 5.0                                 # one offset beyond +-4: the guard sends the call to the exact set
    a = _grads(capi, plan, *far)
    _same_bits(a, _grads(capi, _plan(capi, shape, "bf16", capi.FLAG_NO_DENSE_SPLIT, k=17), *far), "hand-over/far")
    near = _inputs(43, shape, 3.5)
    b = _grads(capi, plan, *near)                        # after a hint of 5
    _same_bits(b, _grads(capi, _plan(capi, shape, "bf16", k=17), *near), "hand-over/near")
    _same_bits(b, _grads(capi, _plan(capi, shape, "f32", capi.FLAG_DENSE_SPLIT_F16, k=17), *near), "hand-over/near-is-the-member")


# ---- 6. the three-product reference build ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, shape, m, seed", [RING_CASES[5], RING_CASES[6]], ids=["ragged", "small-ragged"])
def test_one_limb_error_is_bit_identical_to_the_three_product_build(name, shape, m, seed):
    capi, e2 = _capi(), variant_capi("bf16_e2")
    case = _inputs(seed, shape, m)
    one = _grads(capi, _plan(capi, shape, "bf16"), *case)
    three = _grads(e2, _plan(e2, shape, "bf16"), *case)
    assert e2.Plan(*shape, flags=e2.FLAG_USE_INTERPOLATION | e2.FLAG_IO_BF16).workspace_bytes(e2.PASS_BACKWARD) >= \
        capi.Plan(*shape, flags=capi.FLAG_USE_INTERPOLATION | capi.FLAG_IO_BF16).workspace_bytes(capi.PASS_BACKWARD)
    _same_bits(one, three, "e1-vs-e2/" + name)


# ---- 7. the layer --------------------------------------------------------------------------------------------------------------
def test_bf16_layer_under_autocast_takes_the_member():
    import dau_conv
    import torch.nn as nn
    torch.manual_seed(3)
    conv = nn.Conv2d(3, 32, 3, padding=1).cuda()
    layer = dau_conv.DAUConv2d(filters=32, dau_units=(2, 2), max_kernel_size=9, use_bias=False, in_channels=32,
                               mu1_initializer=dau_conv.random_uniform_initializer(-3, 3),
                               mu2_initializer=dau_conv.random_uniform_initializer(-3, 3), mu_learning_rate_factor=1.0).cuda()
    x = torch.rand(4, 3, 24, 24, device="cuda")
    seen = {}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h = conv(x)
        h.retain_grad()
        y = layer(h)
        y.register_hook(lambda g: seen.__setitem__("dy", g.detach().clone()))
        loss = y.float().pow(2).mean()
    loss.backward()
    dau_conv.check_pending_offsets()
    assert h.dtype == torch.bfloat16 and y.dtype == torch.bfloat16 and h.grad.dtype == torch.bfloat16
    assert seen["dy"].dtype == torch.bfloat16
    grads = {n: getattr(layer, n).grad for n in ("weights", "mu1", "mu2")}
    assert all(g is not None and g.dtype == torch.float32 for g in grads.values())
    # the same bf16-rounded tensors as float32 through the op, the split members forced
    leaves = [getattr(layer, "dau_" + n).detach().clone().requires_grad_(True) for n in ("weights", "mu1", "mu2")]
    sigma = layer._sigma_tensor_and_hint()[0].detach()
    yr = dau_conv.dau_conv(h.detach().float(), *leaves, sigma, num_output=32, number_units_x=2, number_units_y=2, kernel_size=9,
                           mu_learning_rate_factor=1.0, component_border_bound=layer.dau_unit_border_bound, dense_split=True)
    yr.backward(seen["dy"].float())
    for n, leaf in zip(("weights", "mu1", "mu2"), leaves):
        assert torch.equal(grads[n], leaf.grad), n
