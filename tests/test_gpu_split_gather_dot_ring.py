"""GPU: the row ring of the two-limb f16 gather-dot (k_split_dot.hip).  The items of a chunk walk down the column strips of an
image octet; an item copies only the rows its window adds to the previous one, and the whole window at the first item of a
chunk or of a strip.  Each case below is built to reach one corner of that geometry (the geometry is recomputed here and the
case checks it does); the bar is the fp32 one against the oracle, on a slice of output channels where the layer is wide (the
gradients of a unit depend on its own output channel only)."""
import numpy as np
import pytest

from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, record_margins

pytestmark = pytest.mark.gpu

PARAMS = ("dw", "dmu1", "dmu2", "dsigma")


def _geom(N, S, F, G, H, W):
    """the host's region geometry (split_dot_configure / sd_geom)"""
    best, best_cost = 0, None
    for rw in (12, 10):
        wq = -(-(W + 1) // rw) * rw
        cost = wq * (rw + 2) * (60 // rw)
        if best_cost is None or cost < best_cost:
            best, best_cost = rw, cost
    rq = -(-(H + 1) // 4)
    cq = -(-(W + 1) // best)
    items = -(-N // 8) * rq * cq
    per_chunk = -(-F // 16) * -(-S // 16) * -(-G // 4)
    chunks = max(1, min(-(-1024 // per_chunk), items))
    per = -(-items // chunks)
    starts = list(range(0, items, per))
    return dict(RW=best, rq=rq, cq=cq, items=items, per=per, starts=starts, wq=cq * best)


def _run(N, S, F, G, H, W, m, seed, fs=None):
    import torch
    from dau_conv import _capi
    x, dy, w, mu1, mu2 = make_inputs(seed, N, S, F, G, H, W, 9, m)
    # the extreme offsets of the window on the first units
    mu1.flat[0] = m; mu2.flat[0] = -m; mu1.flat[1] = -m; mu2.flat[1] = m
    plan = _capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5,
                      flags=_capi.FLAG_USE_INTERPOLATION | _capi.FLAG_DENSE_SPLIT_F16)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
    need = _capi.NEED_DW | _capi.NEED_DMU1 | _capi.NEED_DMU2 | _capi.NEED_DSIGMA
    g = plan.backward(dev(x), dev(dy), dev(w), dev(mu1), dev(mu2), sg, need_mask=need)
    plan.check_status()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in zip(("dx",) + PARAMS, g) if k in PARAMS}
    fs = np.arange(F) if fs is None else np.asarray(fs)
    want = orc.backward(x, dy[:, fs], w[..., fs], mu1[..., fs], mu2[..., fs], 0.5, need=PARAMS)
    return {k: got[k][..., fs] for k in PARAMS}, want


def _check(name, got, want):
    for key in PARAMS:
        assert_parity(got[key], want[key], name + "/" + key)
    record_margins(name, got, {k: want[k] for k in PARAMS}, "1e-4 rel + 1e-6 max-norm (fp32 bar; split-f16 gather-dot, row ring)")


def _edge_channels(F):
    return sorted(set(range(4)) | set(range(F - 4, F)))


def test_ring_chunk_begins_in_the_middle_of_a_strip():
    N, S, F, G, H, W = 8, 256, 256, 4, 27, 27
    g = _geom(N, S, F, G, H, W)
    assert any(s % g["rq"] for s in g["starts"]) and g["per"] > 1
    _check("ring/mid-strip", *_run(N, S, F, G, H, W, 3.0, 301, _edge_channels(F)))


def test_ring_single_strip():
    N, S, F, G, H, W = 8, 256, 256, 4, 40, 9
    g = _geom(N, S, F, G, H, W)
    assert g["cq"] == 1 and g["per"] > 1 and g["rq"] > g["per"]
    _check("ring/single-strip", *_run(N, S, F, G, H, W, 3.0, 302, _edge_channels(F)))


def test_ring_single_region_row():
    """every item starts a strip: nothing is copied ahead"""
    N, S, F, G, H, W = 16, 256, 256, 4, 3, 40
    g = _geom(N, S, F, G, H, W)
    assert g["rq"] == 1 and g["per"] > 1
    _check("ring/single-row", *_run(N, S, F, G, H, W, 3.0, 303, _edge_channels(F)))


@pytest.mark.parametrize("W, RW", [(35, 12), (29, 10)])
def test_ring_w_plus_one_multiple_of_rw(W, RW):
    N, S, F, G, H = 8, 256, 256, 4, 20
    g = _geom(N, S, F, G, H, W)
    assert g["wq"] == W + 1 and g["RW"] == RW
    _check("ring/exact-columns-%d" % RW, *_run(N, S, F, G, H, W, 3.0, 304, _edge_channels(F)))


def test_ring_ragged_batch_and_channel_blocks():
    """N not a multiple of 8, S and F not multiples of 16, G not a multiple of 4"""
    N, S, F, G, H, W = 13, 250, 100, 7, 20, 20
    g = _geom(N, S, F, G, H, W)
    assert g["per"] > 1 and any(s % g["rq"] for s in g["starts"])
    _check("ring/ragged", *_run(N, S, F, G, H, W, 3.0, 305, _edge_channels(F)))


def test_ring_small_ragged_layer():
    N, S, F, G, H, W = 5, 40, 36, 3, 24, 24
    _check("ring/small-ragged", *_run(N, S, F, G, H, W, 3.0, 306))


@pytest.mark.parametrize("m", [3.99, -3.99])
def test_ring_offsets_at_the_clip(m):
    N, S, F, G, H, W = 8, 256, 256, 4, 32, 32
    g = _geom(N, S, F, G, H, W)
    assert g["per"] > 1 and g["rq"] > 1
    _check("ring/m%+.2f" % m, *_run(N, S, F, G, H, W, m, 307, _edge_channels(F)))
