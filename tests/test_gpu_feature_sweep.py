"""GPU: seeded random shapes through the newer features TOGETHER, against the oracle -- float16 / bfloat16 storage, NHWC, the default
plan's members and the forced ones (DAU_FLAG_NO_DENSE_SPLIT, DAU_FLAG_DENSE_SPLIT_F16, with DAU_FLAG_DENSE_SPLIT_OUTLIERS), the input
ReLU, and the fused bias / ReLU / residual store with dau_conv_epilogue_backward.  tests/feature_sweep.py draws the configurations
(ragged maps, odd channel counts, every reference flag, ignored units, prefilter supports, offsets pinned to the clip and to the
bucket radius itself) and composes the reference; test_feature_sweep_plan.py checks the table on the CPU.  This module is not among
conftest.py's exact-kernel modules and every plan states its flags: the plans are the ones callers get.

One plan per seed, in this order: a plain forward (no hint yet: the static set) against s; the forward with the seed's epilogue (hinted
by the plain call) against y = act((s + bias) + r); epilogue_backward -- dz bit for bit where(y <= 0, 0, dy), dbias within
2^-16 * sum|dz| of the float64 sum; backward on the raw x and that dz, all five gradients; the status after every call, and
outlier_status() == (1, True) after the forward calls and the backward call of an outlier seed.

Bars (none is new): float32 util.assert_parity's defaults; float16 y and dx 2e-3 + 1e-3 of the max-norm (test_gpu_f16.py); bfloat16
y and dx 2e-2 + 4e-3 (test_gpu_bf16.py); the parameter gradients the fp32 bar in every format.

Worst max|err| / max|want| of the 96 default seeds on one MI355X (profiles/r21_parity_margins_feature_sweep.jsonl), y / dx and the
parameter gradients: float32 5.7e-7 (dx, seed 51) and 5.3e-7 (dmu1, seed 18); float16 9.4e-4 (the plain y of seed 64, a four-window
plan: every window pass rounds the stored value again) and 9.2e-7 (dw, seed 7); bfloat16 4.5e-3 (dx of seed 14) and 5.1e-7
(dmu1, seed 71).  With the bias, the residual or the ReLU dropped from the second call, every one of the 48 seeds that has the term fails.

DAU_FUZZ_FEATURE_SEEDS=<n> widens the sweep (default 96)."""
import os

import numpy as np
import pytest
import torch

import feature_sweep as fs
from util import assert_parity, bits as _bits, record_margins

pytestmark = pytest.mark.gpu

DTYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _widened(t):
    return t.float().cpu().numpy()


@pytest.mark.parametrize("seed", range(int(os.environ.get("DAU_FUZZ_FEATURE_SEEDS", str(fs.DEFAULT_SEEDS)))))
def test_random_configuration_with_features(seed):
    from dau_conv import _capi
    cfg = fs.config(seed)
    inp = fs.inputs(cfg)
    N, S, F, G, H, W = fs.shape(cfg)
    dtype = DTYPE[cfg["storage"]]
    fmt = torch.channels_last if cfg["nhwc"] else torch.contiguous_format
    plan = _capi.Plan(N, S, F, G, H, W, **fs.plan_kwargs(cfg))
    assert plan.io_dtype == dtype and plan.io_layout == ("NHWC" if cfg["nhwc"] else "NCHW") and plan.input_relu == cfg["input_relu"]
    act = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).cuda().contiguous(memory_format=fmt)
    dev = lambda a: torch.from_numpy(a).cuda()
    x, dy = act(inp["x"]), act(inp["dy"])
    params = (dev(inp["w"]), dev(inp["mu1"]), dev(inp["mu2"]), torch.full((1, S, G, F), cfg["sigma"], device="cuda"))
    outliers = cfg["members"] == "outliers"
    tag = fs.tag(cfg) + " %s " % {q: cfg[q] for q in ("N", "S", "F", "G", "H", "W", "k", "sigma", "ignore", "c_mode", "c")}

    def status(call):
        plan.check_status()
        if outliers:
            assert plan.outlier_status() == (1, True), "%s: the radius-3 + ring member did not run (%s)" % (tag, call)

    def mine(t, name, like):
        assert t.dtype == dtype and tuple(t.shape) == tuple(like.shape) and t.is_contiguous(memory_format=fmt), "%s: %s is %s %s" % (
            tag, name, t.dtype, t.stride())

    # 1. the plain call: no hint yet, the static set
    y_plain = plan.forward(x, *params)
    status("plain forward")
    # 2. the seed's epilogue: hinted by the plain call
    terms = fs.forward_terms(cfg, inp)
    bias = dev(terms["bias"]) if cfg["bias"] else None
    r = act(terms["r"]) if cfg["residual"] else None
    y = plan.forward(x, *params, bias=bias, relu=cfg["relu"], residual=r)
    status("forward with the epilogue")
    mine(y_plain, "y of the plain call", dy)
    mine(y, "y", dy)
    # 3. the epilogue's backward, from the stored y
    dz = dy
    dbias = None
    if fs.has_epilogue(cfg):               # (a residual alone: nothing to do, the gradient of the sum and of the residual IS dy)
        got_dz, dbias = plan.epilogue_backward(dy, y, relu=cfg["relu"], need_dbias=cfg["bias"])
        if cfg["relu"]:
            mine(got_dz, "dz", dy)
            want_dz = torch.where(y <= 0, torch.zeros_like(dy), dy)
            assert torch.equal(_bits(got_dz), _bits(want_dz)), "%s: %d of %d values of dz differ" % (
                tag, int((_bits(got_dz) != _bits(want_dz)).sum()), dy.numel())
            dz = got_dz
        else:
            assert got_dz is None
        assert (dbias is not None) == cfg["bias"]
    # 4. the backward pass on the raw x and that dz
    grads = plan.backward(x, dz, *params)
    status("backward")
    mine(grads[0], "dx", x)
    for t, key in zip(grads[1:], fs.GRADS):
        assert t.dtype == torch.float32 and tuple(t.shape) == (1, S, G, F) and t.is_contiguous(), "%s: %s" % (tag, key)
    torch.cuda.synchronize()

    want = fs.reference(cfg, inp, _widened(y), terms=terms)
    got = dict(y_plain=_widened(y_plain), y=_widened(y), dx=_widened(grads[0]))
    got.update((key, t.cpu().numpy()) for t, key in zip(grads[1:], fs.GRADS))
    want_all = dict(y_plain=want["s"], **{key: want[key] for key in ("y", "dx") + fs.GRADS})
    rel, floor = fs.BARS[cfg["storage"]]
    m = record_margins("feature_sweep/" + fs.tag(cfg), got, want_all,
                       "y, dx: %g rel + %g max-norm; parameter gradients: 1e-4 + 1e-6" % (rel, floor))
    print(tag, "margins", {key: "%.2e" % v for key, v in m.items()})
    if dbias is not None:
        assert dbias.dtype == torch.float32 and tuple(dbias.shape) == (F,)
        assert np.array_equal(_widened(dz), want["dz"]), tag + "the reference's dz is not the stored one"
        err, bound = np.abs(dbias.double().cpu().numpy() - want["dbias"]), fs.dbias_bound(want["dz"])
        print(tag, "max |dbias - exact| / bound = %.3g" % float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(np.isfinite(err)) and (err <= bound).all(), "%s: |dbias - exact| %s exceeds 2^-16 * sum|dz| %s" % (
            tag, err.tolist(), bound.tolist())
    for key in ("y_plain", "y", "dx"):
        assert_parity(got[key], want_all[key], tag + key, rel=rel, floor=floor)
    for key in fs.GRADS:
        assert_parity(got[key], want_all[key], tag + key)
    if cfg["input_relu"]:
        assert bool((grads[0][x <= 0] == 0).all()), tag + "dx is not masked by the input"
