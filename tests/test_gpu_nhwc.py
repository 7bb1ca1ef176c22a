"""GPU: channels_last activations at the plan level (DAU_FLAG_IO_NHWC).  An NHWC plan is the NCHW plan of the same desc with other
addresses for x, y, dy, dx: the same members, the same arithmetic, the same order of every sum.  So the bar is identity, not a
tolerance: the NHWC call on the permuted tensors returns, bit for bit, the NCHW call's y, dx and parameter gradients -- for every
member and every storage format.  Plus: the project's parity bar against the oracle once, the raw-sums route, and the memory
contract of the C ABI (tests/abi_arena.py) on NHWC arrays, aligned and one element off alignment."""
import numpy as np
import pytest
import torch

import abi_arena as aa
from oracle import dau_oracle as orc
import member_rows as mr
from member_rows import IO, OUTLIERS, inputs as _inputs, nhwc as _nhwc
from util import assert_parity, bits as _bits

pytestmark = pytest.mark.gpu

NAMES = ("y", "dx", "dw", "dmu1", "dmu2", "dsigma")
ROWS = mr.NHWC_ROWS


def _plans(name, io):
    nchw, nhwc = mr.plan(name, io), mr.plan(name, io, nhwc=True)
    assert nhwc.info == nchw.info and nhwc.io_layout == "NHWC"
    return nchw, nhwc


def _run(plan, x, dy, w, mu1, mu2, dtype, outliers=False):
    """forward + backward; x, dy as [N, C, H, W] tensors in the plan's layout -> the six tensors (y, dx in the plan's layout)"""
    dev = lambda a: torch.from_numpy(a).cuda()
    fmt = torch.channels_last if plan.io_layout == "NHWC" else torch.contiguous_format
    xd, dyd = (dev(a).to(dtype).contiguous(memory_format=fmt) for a in (x, dy))
    S, G, F = w.shape[1:]
    sigma = torch.full((1, S, G, F), 0.5, device="cuda")
    wd, m1, m2 = dev(w), dev(mu1), dev(mu2)
    y = plan.forward(xd, wd, m1, m2, sigma)
    plan.check_status()
    if outliers:
        assert plan.outlier_status() == (1, True), "the radius-3 + ring member did not run"
    grads = plan.backward(xd, dyd, wd, m1, m2, sigma)
    plan.check_status()
    return (y,) + tuple(grads)


@pytest.mark.parametrize("io", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", list(ROWS))
def test_nhwc_call_returns_the_bits_of_the_nchw_call(name, io):
    flags = mr.ROWS[name][0]
    nchw, nhwc = _plans(name, io)               # (mr.plan has asserted through Plan.info that each holds the row's member)
    data = _inputs(name)
    want = _run(nchw, *data, dtype=IO[io][1], outliers=bool(flags & OUTLIERS))
    got = _run(nhwc, *data, dtype=IO[io][1], outliers=bool(flags & OUTLIERS))
    for t in got[:2]:
        assert t.is_contiguous(memory_format=torch.channels_last) and t.dtype == IO[io][1]
    for g, r, n in zip(got, want, NAMES):
        assert g.shape == r.shape, n
        differ = int((_bits(g) != _bits(r)).sum())
        assert differ == 0, "%s: %d of %d values differ from the NCHW call" % (n, differ, r.numel())
        assert torch.isfinite(g.float()).all(), n


def test_nhwc_default_plan_against_the_oracle():
    """the project's own bar (util.assert_parity at its defaults), fp32, on the shape whose default plan holds the dense members"""
    _, nhwc = _plans("default_128", "f32")
    x, dy, w, mu1, mu2 = _inputs("default_128")
    got = _run(nhwc, x, dy, w, mu1, mu2, torch.float32)
    want = orc.backward(x, dy, w, mu1, mu2, 0.5)
    want["y"] = orc.forward(x, w, mu1, mu2, 0.5)
    for g, n in zip(got, NAMES):
        assert_parity(g.contiguous().cpu().numpy(), want[n], n)


@pytest.mark.parametrize("io", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["split_17x13_m3", "exact_stacked_28x28", "default_128"])
def test_param_sums_route_gives_the_bits_of_backward(name, io):
    _, nhwc = _plans(name, io)
    xd, dyd = (mr.act(torch.from_numpy(a).cuda(), IO[io][1], nhwc) for a in _inputs(name)[:2])
    wd, m1, m2, sigma = mr.params(name)
    want = nhwc.backward(xd, dyd, wd, m1, m2, sigma)[1:]
    sums = nhwc.backward_param_sums(xd, dyd, m1, m2, sigma)
    got = nhwc.finalize_param_grads(sums, wd)
    nhwc.check_status()
    for g, r, n in zip(got, want, NAMES[2:]):
        assert torch.equal(g.view(torch.int32), r.view(torch.int32)), n


# ---- the memory contract on NHWC arrays: canaries, poisoned outputs and workspace, bases one element off alignment ---------------
_ARENA_FIRST = {}        # (shape name, io, entry point) -> {output: bits} of the first variant that ran


@pytest.mark.parametrize("skew, fill", [(0, 0xFF), (1, 0x7B), (1, 0xFF)])
@pytest.mark.parametrize("io", ["f32", "f16"])
@pytest.mark.parametrize("name", ["split_17x13_m3", "split_tall_28x28"])     # element access only (S = 7); 16-byte loads and stores
def test_memory_contract(name, io, skew, fill):
    """forward, backward and sums + finalize in arenas of their own.  With skew 1 the activation bases are one element off their
    alignment, so the 16-byte paths of the second shape fall back to element access: the same bits."""
    from dau_conv import _capi
    nchw, nhwc = _plans(name, io)
    x, dy, w, mu1, mu2 = _inputs(name)
    S, G, F = w.shape[1:]
    N, H, W = x.shape[0], x.shape[2], x.shape[3]
    params = dict(w=w, mu1=mu1, mu2=mu2, sigma=np.full((1, S, G, F), 0.5, np.float32))
    inputs = dict(params, x=_nhwc(x), dy=_nhwc(dy))
    reports = dict(forward=aa.forward(_capi, nhwc, inputs, io, skew, fill), backward=aa.backward(_capi, nhwc, inputs, io, skew, fill),
                   sums=aa.param_sums_finalize(_capi, nhwc, inputs, io, skew, fill))
    for entry, rep in reports.items():
        tag = "%s %s %s skew %d fill %#x" % (name, io, entry, skew, fill)
        assert rep.rc == _capi.DAU_OK and rep.status_rc == _capi.DAU_OK, "%s: %s" % (tag, _capi.lib.dau_conv_last_error())
        rep.assert_clean(tag)
        for n, v in rep.values.items():
            assert np.isfinite(v).all(), "%s: %s holds non-finite values (poison read, or not overwritten in full)" % (tag, n)
        bits = {n: aa.as_bits(a) for n, a in rep.outputs.items()}
        first = _ARENA_FIRST.setdefault((name, io, entry), bits)
        for n in bits:
            assert np.array_equal(bits[n], first[n]), "%s: %s differs from the first variant's" % (tag, n)
    for n in aa.GRADS:
        assert np.array_equal(aa.as_bits(reports["sums"].outputs[n]), aa.as_bits(reports["backward"].outputs[n])), n
    if skew == 0:
        # and the NCHW plan's arena run on the unpermuted arrays: the same bits, permuted (the arena reports y, dx in the shape
        # [N, C, H, W] whatever they hold: an NHWC result is re-read as [N, H, W, C])
        ref_in = dict(params, x=x, dy=dy)
        ref = dict(forward=aa.forward(_capi, nchw, ref_in, io, 0, fill), backward=aa.backward(_capi, nchw, ref_in, io, 0, fill))
        y = reports["forward"].outputs["y"].reshape(N, H, W, F).transpose(0, 3, 1, 2)
        dx = reports["backward"].outputs["dx"].reshape(N, H, W, S).transpose(0, 3, 1, 2)
        assert np.array_equal(aa.as_bits(np.ascontiguousarray(y)), aa.as_bits(ref["forward"].outputs["y"]))
        assert np.array_equal(aa.as_bits(np.ascontiguousarray(dx)), aa.as_bits(ref["backward"].outputs["dx"]))
        for n in aa.GRADS:
            assert np.array_equal(aa.as_bits(reports["backward"].outputs[n]), aa.as_bits(ref["backward"].outputs[n])), n
