"""GPU: the opt-in radius-3 + ring gather-sum member (DAU_FLAG_DENSE_SPLIT_OUTLIERS).  A call whose offsets reach into (3, 4] in few
units keeps the 7 x 7 two-limb GEMM (k_dense_split.hip, namespace s3) for its y and dx passes; the corners of those units that land
on the ring |tap| = 4 are gathered by the list-driven pass of k_dense_ring.hip, whose fp32 sums join the GEMM's before the one
rounding of the store.  Bar: the fp32 one against the oracle (util.assert_parity defaults: 1e-4 relative + 1e-6 of the max-norm) --
the member claims the accuracy of the radius-3 form, so it gets no bar of its own; margins are recorded with util.record_margins.
dau_conv_gather_outlier_status proves which path a call took.  Replaces the same reference code as the exact gather
(dau_conv_forward_core.hpp:804-1605)."""
import numpy as np
import pytest
import torch

from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, record_margins

pytestmark = pytest.mark.gpu

BAR = "1e-4 rel + 1e-6 max-norm (fp32 bar; radius-3 two-limb GEMM + ring pass)"
GRADS = ("dw", "dmu1", "dmu2", "dsigma")


def _flags(on=True, extra=0, interp=True):
    from dau_conv import _capi
    return ((_capi.FLAG_USE_INTERPOLATION if interp else 0) | _capi.FLAG_DENSE_SPLIT_F16 | (_capi.FLAG_DENSE_SPLIT_OUTLIERS if on else 0) | extra)


def _plan(shape, on=True, extra=0, interp=True, capi=None, **kw):
    if capi is None:
        from dau_conv import _capi as capi
    N, S, F, G, H, W = (shape[q] for q in ("N", "S", "F", "G", "H", "W"))
    plan = capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5, flags=_flags(on, extra, interp), **kw)
    assert plan.info["gather_dense_split"] == (0b111100 if on else 0b011100)
    return plan


def _run(plan, x, dy, w, mu1, mu2, dtype=torch.float32):
    """forward + backward -> (tensors as numpy fp32 (y, dx also raw), outlier status after the forward call, after the backward call)"""
    dev = lambda a: torch.from_numpy(a).cuda()
    S, G, F = w.shape[1:]
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
    xd, dyd = dev(x).to(dtype), dev(dy).to(dtype)
    wd, m1, m2 = dev(w), dev(mu1), dev(mu2)
    y = plan.forward(xd, wd, m1, m2, sg)
    plan.check_status()
    st_f = plan.outlier_status()
    g = plan.backward(xd, dyd, wd, m1, m2, sg)
    plan.check_status()
    st_b = plan.outlier_status()
    torch.cuda.synchronize()
    out = dict(y=y.float().cpu().numpy(), dx=g[0].float().cpu().numpy(), dw=g[1].cpu().numpy(), dmu1=g[2].cpu().numpy(),
               dmu2=g[3].cpu().numpy(), dsigma=g[4].cpu().numpy())
    out["raw"] = dict(y=y.cpu(), dx=g[0].cpu())
    return out, st_f, st_b


def _oracle(x, dy, w, mu1, mu2, **kw):
    want = orc.backward(x, dy, w, mu1, mu2, 0.5, **kw)
    want["y"] = orc.forward(x, w, mu1, mu2, 0.5, **kw)
    return want


def _count(mu1, mu2, ignore=0):
    G = mu1.shape[2]
    return int((np.maximum(np.abs(mu1), np.abs(mu2))[:, :, :G - ignore, :] > 3).sum())


def _out(rs, n):
    """n offsets in +-(3, 3.99]"""
    return (rs.uniform(3.0, 3.99, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32).clip(-3.99, 3.99)


def _outliers(rs, mu1, mu2, pattern):
    """redraw some units of a U(-3, 3) draw into +-(3, 3.99] (in place)"""
    _, S, G, F = mu1.shape
    units = mu1.size
    if pattern == "one":
        (mu1 if rs.rand() < 0.5 else mu2).flat[rs.randint(units)] = _out(rs, 1)[0]
    elif pattern == "percent":
        idx = rs.choice(units, max(2, units // 100), replace=False)
        for i in idx:
            axis = rs.randint(3)                               # mu1, mu2, both
            if axis != 1: mu1.flat[i] = _out(rs, 1)[0]
            if axis != 0: mu2.flat[i] = _out(rs, 1)[0]
    elif pattern == "both_axes":
        idx = rs.choice(units, 4, replace=False)
        for j, i in enumerate(idx):                            # the four corners of the 9 x 9 kernel
            mu1.flat[i] = abs(_out(rs, 1)[0]) * (1 if j & 1 else -1)
            mu2.flat[i] = abs(_out(rs, 1)[0]) * (1 if j & 2 else -1)
    elif pattern == "pair":
        s, f = rs.randint(S), rs.randint(F)
        mu1[0, s, :, f] = _out(rs, G)
        mu2[0, s, :, f] = np.where(rs.rand(G) < 0.5, _out(rs, G), mu2[0, s, :, f])
        if G > 1:
            mu1[0, s, 1, f] = mu1[0, s, 0, f]                  # two units of the pair on the same ring taps: summed in unit order
            mu2[0, s, 1, f] = mu2[0, s, 0, f]
    elif pattern == "exact4":
        i, j = rs.choice(units, 2, replace=False)
        mu1.flat[i] = 4.0
        mu2.flat[j] = -4.0
    else:
        raise ValueError(pattern)


# (the member takes calls with at most 1 % of the plan's live units beyond +-3: every pattern below stays within that on every shape)
SHAPES = [
    dict(N=2, S=20, F=40, G=3, H=27, W=27),       # 24 + 3 rows, odd width; channels ragged against 16 and 128
    dict(N=2, S=16, F=130, G=4, H=28, W=28),      # the four-row block / tall tiles' map; two GEMM channel blocks, three of the ring pass
    dict(N=2, S=24, F=72, G=6, H=56, W=56),       # the north-star map; two ring channel blocks, the second of eight channels
    dict(N=1, S=33, F=16, G=1, H=20, W=100),      # two column blocks of the ring pass; a third chunk of one channel
    dict(N=3, S=23, F=9, G=5, H=12, W=14),        # small map, a ragged second chunk, odd batch
    dict(N=2, S=48, F=64, G=2, H=20, W=100),
]
PATTERNS = ["one", "percent", "both_axes", "pair", "exact4"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_g%d" % (s["H"], s["W"], s["G"]))
def test_ring_member_against_oracle(shape, pattern):
    N, S, F, G, H, W = (shape[q] for q in ("N", "S", "F", "G", "H", "W"))
    seed = 7 + PATTERNS.index(pattern) + 10 * SHAPES.index(shape)
    x, dy, w, mu1, mu2 = make_inputs(seed, N, S, F, G, H, W, 9, 3.0)
    _outliers(np.random.RandomState(seed + 1000), mu1, mu2, pattern)
    count = _count(mu1, mu2)
    assert count >= 1 and max(np.abs(mu1).max(), np.abs(mu2).max()) > 3
    got, st_f, st_b = _run(_plan(shape), x, dy, w, mu1, mu2)
    want = _oracle(x, dy, w, mu1, mu2)
    name = "outliers/%s/%dx%d_g%d" % (pattern, H, W, G)
    m = record_margins(name, {k: got[k] for k in want}, want, BAR)
    print(name, "outlier units", count, "margins", {k: "%.2e" % v for k, v in m.items()})
    for key in ("y", "dx") + GRADS:
        assert_parity(got[key], want[key], name + "/" + key)
    # the path: the device counted the outlier units and the ring member did both gather-sum passes
    assert st_f == (count, True), (st_f, count)
    assert st_b == (count, True), (st_b, count)
    # the parameter-gradient pass is not affected
    ref, rf, rb = _run(_plan(shape, on=False), x, dy, w, mu1, mu2)
    assert rf == (count, False) and rb == (count, False)
    for key in GRADS:
        assert np.array_equal(got[key], ref[key]), key
    # deterministic: a second call gives the same bits
    again, _, _ = _run(_plan(shape), x, dy, w, mu1, mu2)
    for key in ("y", "dx"):
        assert np.array_equal(got[key], again[key]), key


@pytest.mark.parametrize("shape", SHAPES[:4], ids=lambda s: "%dx%d_g%d" % (s["H"], s["W"], s["G"]))
def test_inlier_calls_and_calls_above_the_limit_run_what_they_ran(shape):
    """max|mu| <= 3: the radius-2 / radius-3 members as without the flag.  More outlier units than the limit (U(-3.99, 3.99): 44 % of
    the units): the radius-4 member as without the flag.  Bit-identical y and dx, ring not taken."""
    N, S, F, G, H, W = (shape[q] for q in ("N", "S", "F", "G", "H", "W"))
    on, off = _plan(shape), _plan(shape, on=False)
    for m, label in ((3.0, "inliers"), (3.99, "above the limit")):
        x, dy, w, mu1, mu2 = make_inputs(91, N, S, F, G, H, W, 9, m)
        count = _count(mu1, mu2)
        assert (count == 0) if m == 3.0 else (count > 0.3 * mu1.size)
        got, st_f, st_b = _run(on, x, dy, w, mu1, mu2)
        ref, _, _ = _run(off, x, dy, w, mu1, mu2)
        assert st_f == (count, False) and st_b == (count, False), (label, st_f, st_b, count)
        for key in ("y", "dx") + GRADS:
            assert np.array_equal(got[key], ref[key]), (label, key)
    # ... and a call decides for itself, whatever the plan ran before: few outliers right after many
    x, dy, w, mu1, mu2 = make_inputs(92, N, S, F, G, H, W, 9, 3.0)
    mu1.flat[3] = 3.7
    got, st_f, st_b = _run(on, x, dy, w, mu1, mu2)
    assert st_f == (1, True) and st_b == (1, True)
    want = _oracle(x, dy, w, mu1, mu2)
    for key in ("y", "dx"):
        assert_parity(got[key], want[key], "after-many/" + key)


def test_float16_io_rounds_once():
    """y (dx) of the float16 plan = the f16 rounding of the fp32 plan's y (dx) on the widened input, bit for bit: the ring sums join
    the GEMM's in fp32, before the store's one rounding."""
    from dau_conv import _capi
    shape = dict(N=2, S=20, F=40, G=3, H=27, W=27)
    x, dy, w, mu1, mu2 = make_inputs(5, 2, 20, 40, 3, 27, 27, 9, 3.0)
    _outliers(np.random.RandomState(6), mu1, mu2, "percent")
    x16, dy16 = x.astype(np.float16), dy.astype(np.float16)
    got, st_f, st_b = _run(_plan(shape, extra=_capi.FLAG_IO_F16), x16.astype(np.float32), dy16.astype(np.float32), w, mu1, mu2, torch.float16)
    ref, _, _ = _run(_plan(shape), x16.astype(np.float32), dy16.astype(np.float32), w, mu1, mu2)
    count = _count(mu1, mu2)
    assert st_f == (count, True) and st_b == (count, True)
    assert got["raw"]["y"].dtype == torch.float16
    for key in ("y", "dx"):
        want16 = ref["raw"][key].to(torch.float16)
        assert torch.equal(got["raw"][key].view(torch.int16), want16.view(torch.int16)), key
    for key in GRADS:
        assert np.array_equal(got[key], ref[key]), key


def test_bfloat16_io():
    from dau_conv import _capi
    shape = dict(N=2, S=20, F=40, G=3, H=28, W=28)
    x, dy, w, mu1, mu2 = make_inputs(8, 2, 20, 40, 3, 28, 28, 9, 3.0)
    _outliers(np.random.RandomState(9), mu1, mu2, "percent")
    xb = torch.from_numpy(x).to(torch.bfloat16).float().numpy()          # what the kernels read
    dyb = torch.from_numpy(dy).to(torch.bfloat16).float().numpy()
    got, st_f, st_b = _run(_plan(shape, extra=_capi.FLAG_IO_BF16), xb, dyb, w, mu1, mu2, torch.bfloat16)
    count = _count(mu1, mu2)
    assert st_f == (count, True) and st_b == (count, True)
    want = _oracle(xb, dyb, w, mu1, mu2)
    # the bar of tests/test_gpu_bf16.py for bf16 storage: half an ulp of bfloat16 per rounding, one rounding
    for key in ("y", "dx"):
        assert_parity(got[key], want[key], "bf16/" + key, rel=2e-2, floor=4e-3)


def test_batch_slabs(monkeypatch):
    """A workspace budget that forces the gather-sum passes to run slab by slab: the list is built once, the ring pass and the GEMM run
    per slab over the slab's partial sums."""
    shape = dict(N=8, S=20, F=40, G=3, H=27, W=27)
    monkeypatch.setenv("DAU_WORKSPACE_BUDGET_GB", "0.0005")
    plan = _plan(shape)
    monkeypatch.delenv("DAU_WORKSPACE_BUDGET_GB")
    assert plan.info["batch_slab_gather"] < 8, plan.info
    x, dy, w, mu1, mu2 = make_inputs(12, 8, 20, 40, 3, 27, 27, 9, 3.0)
    _outliers(np.random.RandomState(13), mu1, mu2, "percent")
    got, st_f, st_b = _run(plan, x, dy, w, mu1, mu2)
    count = _count(mu1, mu2)
    assert st_f == (count, True) and st_b == (count, True)
    want = _oracle(x, dy, w, mu1, mu2)
    for key in ("y", "dx") + GRADS:
        assert_parity(got[key], want[key], "slabs/" + key)
    whole, _, _ = _run(_plan(shape), x, dy, w, mu1, mu2)              # per-image passes: the same bits as the whole batch at once
    for key in ("y", "dx"):
        assert np.array_equal(got[key], whole[key]), key


@pytest.mark.parametrize("form", ["no_interpolation", "single_dim", "units_ignore"])
def test_other_unit_table_forms(form):
    from dau_conv import _capi
    shape = dict(N=2, S=20, F=40, G=4, H=20, W=30)
    ignore = 1 if form == "units_ignore" else 0
    x, dy, w, mu1, mu2 = make_inputs(21, 2, 20, 40, 4, 20, 30, 9, 3.0, ignore=ignore)
    rs = np.random.RandomState(22)
    # (the count limit is 1 % of the LIVE units: with ignored units, a pattern of a few units)
    _outliers(rs, mu1, mu2, "both_axes" if ignore else "percent")
    if ignore:
        mu1[0, 1, 0, 2], mu2[0, 5, 1, 7] = 3.6, -3.3                  # live units, whatever the pattern drew
    kw, extra, okw = {}, 0, {}
    if form == "no_interpolation":
        okw = dict(use_interpolation=False)
    elif form == "single_dim":
        mu2[:] = 0.0                                                  # (the units the pattern moved along mu1 stay outliers)
        extra, okw = _capi.FLAG_SINGLE_DIM_KERNEL, dict(single_dim_kernel=True)
    else:
        mu1[0, :, 3, ::5] = 3.5                                       # ignored units beyond +-3 too: they do not count
        kw, okw = dict(number_units_ignore=1), dict(ignore=1)
    count = _count(mu1, mu2, ignore)
    assert count >= 1 and (ignore == 0 or count < _count(mu1, mu2))
    plan = _plan(shape, extra=extra, interp=form != "no_interpolation", **kw)
    got, st_f, st_b = _run(plan, x, dy, w, mu1, mu2)
    assert st_f == (count, True) and st_b == (count, True), (st_f, st_b, count)
    want = _oracle(x, dy, w, mu1, mu2, **okw)
    for key in ("y", "dx") + GRADS:
        assert_parity(got[key], want[key], form + "/" + key)
    ref, _, _ = _run(_plan(shape, on=False, extra=extra, interp=form != "no_interpolation", **kw), x, dy, w, mu1, mu2)
    for key in GRADS:
        assert np.array_equal(got[key], ref[key]), key


def test_depth_256_channels():
    """S = F = 256 at the north-star map, 1 % outlier units: the distance to the bar with 16 chunks of accumulation behind every output
    (the radius-3 member alone: 4.0e-7 of the max-norm)."""
    from dau_conv import _capi
    shape = dict(N=4, S=256, F=256, G=4, H=56, W=56)
    x, dy, w, mu1, mu2 = make_inputs(31, 4, 256, 256, 4, 56, 56, 9, 3.0)
    rs = np.random.RandomState(32)
    idx = rs.choice(mu1.size, mu1.size // 100, replace=False)
    mu1.flat[idx[::2]] = _out(rs, len(idx[::2]))
    mu2.flat[idx[1::2]] = _out(rs, len(idx[1::2]))
    count = _count(mu1, mu2)
    plan = _capi.Plan(4, 256, 256, 4, 56, 56, max_kernel_size=9, sigma_hint=0.5, flags=_capi.FLAG_USE_INTERPOLATION | _capi.FLAG_DENSE_SPLIT_OUTLIERS)
    assert plan.info["gather_dense_split"] == 0b111100              # the default plan of this shape, plus the opt-in
    got, st_f, st_b = _run(plan, x, dy, w, mu1, mu2)
    assert st_f == (count, True) and st_b == (count, True)
    want = _oracle(x, dy, w, mu1, mu2)
    m = record_margins("outliers/depth/256x256_56x56_p1", {k: got[k] for k in want}, want, BAR)
    print("depth margins", {k: "%.2e" % v for k, v in m.items()}, "outlier units", count)
    for key in ("y", "dx") + GRADS:
        assert_parity(got[key], want[key], "depth/" + key)


def test_layer_trains_at_the_clip():
    """DAUConv2d(dense_outliers=True) with offsets pushed to the +-3.99 clip of kernel 9: a few SGD steps; its plan holds the member and
    takes it; forward and backward agree with a dense_outliers=False layer of the same parameters within the bar."""
    import importlib
    import dau_conv
    dc = importlib.import_module("dau_conv.dau_conv")
    dc._PLANS.clear()
    torch.manual_seed(3)

    def make(flag):
        return dau_conv.DAUConv2d(filters=128, dau_units=(2, 2), max_kernel_size=9, use_bias=False, in_channels=128,
                                  mu1_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                  mu2_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                  mu_learning_rate_factor=1.0, dense_outliers=flag).cuda()
    on, off = make(True), make(False)
    with torch.no_grad():
        pick = torch.rand_like(on.dau_mu1) < 0.004                     # (the member's count limit is 1 % of the units)
        on.dau_mu1[pick] = 7.0                                         # beyond the kernel: the layer clips them to 3.99
        on.dau_mu2[torch.rand_like(on.dau_mu2) < 0.002] = -7.0
    off.load_state_dict(on.state_dict())
    x = torch.rand(2, 128, 16, 16, device="cuda")
    dy = torch.randn(2, 128, 16, 16, device="cuda")
    opts = [torch.optim.SGD(l.parameters(), lr=1e-3) for l in (on, off)]
    for step in range(3):
        outs = []
        for layer, opt in ((on, opts[0]), (off, opts[1])):
            opt.zero_grad()
            xi = x.clone().requires_grad_(True)
            y = layer(xi)
            y.backward(dy)
            if layer is on:
                # (every plan of a stream shares one workspace: ask before the other layer's calls overwrite the status block)
                plans = [p for p in dc._PLANS.values() if p.info["gather_dense_split"] & (1 << 5)]
                assert len(plans) == 1
                units, taken = plans[0].outlier_status()
                assert taken and 0 < units <= on.dau_mu1.numel() // 100, (step, units, taken)
            outs.append(dict(y=y.detach().cpu().numpy(), dx=xi.grad.cpu().numpy(), dw=layer.dau_weights.grad.cpu().numpy(),
                             dmu1=layer.dau_mu1.grad.cpu().numpy(), dmu2=layer.dau_mu2.grad.cpu().numpy()))
        dau_conv.check_pending_offsets()
        for key in outs[0]:
            assert_parity(outs[0][key], outs[1][key], "layer/step%d/%s" % (step, key))
        for opt in opts:
            opt.step()
        with torch.no_grad():                                          # keep the two layers on the same parameters
            off.load_state_dict(on.state_dict())
    assert len(dc._PLANS) == 2
    dc._PLANS.clear()
