"""CPU: the configurations of tests/feature_sweep.py (GPU: test_gpu_feature_sweep.py) -- that config(seed) is a function of the
seed alone, that every seed's plan is created for its flags and holds what the seed names, that the table of the default seed count
covers what it is meant to cover (a condition, not a measurement), that the inputs can fail a kernel which forgets a term, and
the composition of the reference against torch's autograd.  Plan creation needs no device; nothing is launched here.

The power of the inputs runs the oracle's forward pass for every seed (a few seconds in all: no seed is left out).  "The bar at the
max-norm" is the absolute term of util.assert_parity, floor * max|y_ref|: the distance every element is allowed whatever its size."""
import collections
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feature_sweep as fs
import util

SEEDS = range(fs.DEFAULT_SEEDS)
RING = 1 << 5


def _plan(cfg):
    from dau_conv import _capi
    return _capi, _capi.Plan(*fs.shape(cfg), **fs.plan_kwargs(cfg))


_INFO = {}


def _info(seed):
    if seed not in _INFO:
        _INFO[seed] = _plan(fs.config(seed))[1].info
    return _INFO[seed]


def test_flag_values_are_the_bindings():
    from dau_conv import _capi
    for name in ("FLAG_USE_INTERPOLATION", "FLAG_UNIT_TESTING", "FLAG_SINGLE_DIM_KERNEL", "FLAG_FORBID_POSITIVE_DIM1", "FLAG_IO_BF16",
                 "FLAG_IO_F16", "FLAG_IO_NHWC", "FLAG_INPUT_RELU", "FLAG_DENSE_SPLIT_F16", "FLAG_NO_DENSE_SPLIT",
                 "FLAG_DENSE_SPLIT_OUTLIERS", "EPILOGUE_BIAS", "EPILOGUE_RELU"):
        assert getattr(fs, name) == getattr(_capi, name), name


# ---- determinism -------------------------------------------------------------------------------------------------------------------

def test_config_is_a_function_of_the_seed():
    dump = lambda: json.dumps([fs.config(s) for s in SEEDS], sort_keys=True)
    here = dump()
    assert here == dump()
    code = "import json, feature_sweep as fs; print(json.dumps([fs.config(s) for s in range(%d)], sort_keys=True))" % len(SEEDS)
    env = dict(os.environ, PYTHONHASHSEED="random")
    fresh = subprocess.check_output([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)), env=env)
    assert fresh.decode().strip() == here
    a, b = fs.inputs(fs.config(5)), fs.inputs(fs.config(5))
    assert all(np.array_equal(a[key], b[key]) for key in a)


def test_configurations_stay_within_the_fuzz_ranges():
    for cfg in map(fs.config, SEEDS):
        N, S, F, G, H, W = fs.shape(cfg)
        assert 1 <= N <= 5 and 1 <= S <= 40 and 1 <= F <= 70 and G in (1, 2, 3, 4, 5, 6, 8, 9) and 0 <= cfg["ignore"] < G
        assert (5 <= H <= 79 and 5 <= W <= 79) or (cfg["seed"] % 7 == 0 and H in (56, 64, 96, 112) and W in (56, 64, 72, 120))
        assert cfg["k"] in (9, 17, 33, 37, 41, 49, 65)
        dense = cfg["members"] in ("split", "outliers")
        assert cfg["sigma"] <= (1.0 if dense else 1.4)
        inp = fs.inputs(cfg)
        top = max(np.abs(inp["mu1"]).max(), np.abs(inp["mu2"]).max())
        assert top <= cfg["k"] // 2, "an offset beyond what the plan's kernel size allows"
        assert inp["mu1"].flat[0] == np.float32(cfg["c"]) and (cfg["flags"]["single_dim_kernel"] or inp["mu2"].flat[0] == np.float32(-cfg["c"]))
        if cfg["members"] == "outliers":
            assert cfg["flags"]["use_interpolation"] and cfg["sigma"] <= 1.0 and cfg["c"] <= 3.0 and fs.outlier_units(cfg, inp) == 1
            assert np.sort(np.abs(np.concatenate([inp["mu1"].ravel(), inp["mu2"].ravel()])))[-2] <= 3.0 and top == fs.OUTLIER_OFFSET
        elif dense:
            assert top <= 4.0
        if cfg["c_mode"] == "bucket":
            assert cfg["c"] == fs.bucket_of(cfg["m"]) == top and cfg["members"] != "outliers"
        if cfg["c_mode"] == "integer":
            assert cfg["c"] == int(cfg["c"]) <= cfg["m"]
        # x and dy are what the storage format holds
        for key in ("x", "dy"):
            assert np.array_equal(fs.rounded(inp[key], cfg["storage"]), inp[key])


# ---- every seed's plan -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_seed_plan(seed):
    cfg = fs.config(seed)
    capi, plan = _plan(cfg)
    info = plan.info
    assert info["algo_forward"] == info["algo_backward"] == capi.ALGO_TILED, info
    assert plan.epilogue_supported(fs.epilogue_bits(cfg)) if fs.epilogue_bits(cfg) else True
    if cfg["residual"]:
        assert plan._residual_supported()
    assert plan.io_layout == ("NHWC" if cfg["nhwc"] else "NCHW") and plan.input_relu == cfg["input_relu"]
    assert plan.io_dtype == {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[cfg["storage"]]
    assert info["offset_bucket"] == fs.bucket_of(cfg["k"] // 2)
    split = info["gather_dense_split"]
    if cfg["members"] == "split":
        assert split == 0b11100, bin(split)
    elif cfg["members"] == "outliers":
        assert split == 0b11100 | RING, bin(split)
        # the one outlier fits the member's limit of 1 % of the live units
        assert cfg["S"] * cfg["F"] * (cfg["G"] - cfg["ignore"]) // 100 >= 1
    elif cfg["members"] == "exact":
        assert split == 0
    else:
        assert not split & RING


# ---- coverage of the table ---------------------------------------------------------------------------------------------------------

def test_every_pair_of_feature_values_occurs_twice():
    fts = [fs.features(s) for s in SEEDS]
    for cfg, ft in zip(map(fs.config, SEEDS), fts):                # config() carries the table's values
        assert (cfg["storage"], cfg["nhwc"], cfg["members"], cfg["input_relu"], cfg["epilogue"]) == (
            ft["storage"], ft["layout"] == "nhwc", ft["members"], ft["input_relu"], ft["epilogue"])
    for a, b in itertools.combinations(fs.FEATURES, 2):
        count = collections.Counter((ft[a], ft[b]) for ft in fts)
        for pair in itertools.product(fs.FEATURES[a], fs.FEATURES[b]):
            assert count[pair] >= 2, "%s x %s: %s occurs %d times" % (a, b, pair, count[pair])
    # and all of them at once exactly once in 384 consecutive seeds
    assert len({tuple(fs.features(s).values()) for s in range(384)}) == 384


def test_the_combinations_nobody_wrote_into_a_table_occur_twice():
    count = collections.Counter()
    for cfg in map(fs.config, SEEDS):
        info = _info(cfg["seed"])
        if info["gather_windows"] > 1 and fs.has_epilogue(cfg): count["windows with an epilogue"] += 1
        if info["gather_windows"] > 1 and cfg["input_relu"]: count["windows with the input ReLU"] += 1
        if cfg["unit_testing"] and cfg["residual"]: count["unit_testing with a residual"] += 1
        if not cfg["flags"]["use_interpolation"] and cfg["input_relu"]: count["interpolation off with the input ReLU"] += 1
        if cfg["c_mode"] == "bucket":
            count["pinned to R = %s" % ("16..32" if cfg["c"] >= 16 else "%d" % cfg["c"])] += 1
        # by default the split gather-dot is held where the blocks of four units are at least 3/4 full; no field of the plan info
        # names it: a plan that holds it asks for another backward workspace than its NO_DENSE_SPLIT twin
        if cfg["members"] == "default" and cfg["G"] in (3, 4, 7, 8) and _holds_split_dot(cfg): count["default plan with the split gather-dot"] += 1
    for what in ("windows with an epilogue", "windows with the input ReLU", "unit_testing with a residual",
                 "interpolation off with the input ReLU", "pinned to R = 4", "pinned to R = 8", "pinned to R = 16..32",
                 "default plan with the split gather-dot"):
        assert count[what] >= 2, "%s: %d seeds" % (what, count[what])


def _holds_split_dot(cfg):
    from dau_conv import _capi
    kw = fs.plan_kwargs(cfg)
    mine = _capi.Plan(*fs.shape(cfg), **kw).workspace_bytes(_capi.PASS_BACKWARD)
    kw["flags"] |= fs.FLAG_NO_DENSE_SPLIT
    return mine != _capi.Plan(*fs.shape(cfg), **kw).workspace_bytes(_capi.PASS_BACKWARD)


# ---- power of the inputs (the oracle alone) ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_power_of_the_inputs(seed):
    """Input-ReLU seeds: between 0.2 and 0.8 of x is <= 0.  ReLU seeds: between 0.2 and 0.8 of y_ref is <= 0.  Bias and residual seeds:
    y_ref without the term lies more than 100 times the bar at the max-norm from y_ref, and fails the very comparison the GPU test
    makes of y.  The helper draws the bias conditioned on this (forward_terms): a first draw of eight bfloat16 bias seeds moved y by 56
    to 89 bars only -- 4e-3 * max|y_ref| is a wide bar, and a residual in the same sum widens it -- and their second to twelfth does."""
    cfg = fs.config(seed)
    if not (cfg["input_relu"] or fs.has_epilogue(cfg)):
        return
    inp = fs.inputs(cfg)
    if cfg["input_relu"]:
        share = float((inp["x"] <= 0).mean())
        assert 0.2 < share < 0.8, "%.2f of x is <= 0: the clamp would not show" % share
    if not fs.has_epilogue(cfg):
        return
    t = fs.forward_terms(cfg, inp)
    y = t["y"]
    if cfg["relu"]:
        share = float((y <= 0).mean())
        assert 0.2 < share < 0.8, "ReLU cuts %.2f of y_ref" % share
    if cfg["bias"]:
        # the conditioned draw ended because a draw passed, and did not start where the first draw has margin to spare
        assert t["bias_draws"] < fs.BIAS_DRAWS and (cfg["storage"] == "bf16" or t["bias_draws"] == 1), t["bias_draws"]
        assert t["bias"].dtype == np.float32 and t["bias"].shape == (cfg["F"],)
    rel, floor = fs.BARS[cfg["storage"]]
    bar = floor * np.abs(y).max()
    for term, without in (("bias", fs.compose(t["s"], None, t["r"], cfg["relu"])), ("residual", fs.compose(t["s"], t["bias"], None, cfg["relu"]))):
        if cfg[term]:
            moved = float(np.abs(without - y).max())
            over = util.parity_error(without, y, rel, floor)
            print("%s: without the %s y_ref moves by %.3g = %.3g x the bar at the max-norm (draw %d of the bias); the comparison of y is "
                  "violated by %.3g x it" % (fs.tag(cfg), term, moved, moved / bar, t["bias_draws"], over / bar))
            assert moved > 100 * bar, "%s: a kernel that forgets the %s moves y by %.3g = %.3g x the bar at the max-norm %.3g" % (
                fs.tag(cfg), term, moved, moved / bar, bar)
            assert over > 0, "%s: y without the %s passes the comparison the GPU test makes" % (fs.tag(cfg), term)
            assert abs(fs.power(cfg, t["s"], t["bias"], t["r"])[term] - moved / bar) <= 1e-9 * moved / bar


def test_the_bias_is_drawn_at_the_size_of_s():
    """conditioning leaves the draw what it is: over the bias seeds, bias / std(s) has the spread of a standard normal (within the
    sampling error of some 1500 values, the conditioned seeds' one large channel each included)"""
    ratios = []
    for cfg in map(fs.config, SEEDS):
        if cfg["bias"]:
            t = fs.forward_terms(cfg, fs.inputs(cfg))
            ratios.append(t["bias"].astype(np.float64) / np.asarray(t["s"], np.float64).std())
    ratios = np.concatenate(ratios)
    assert ratios.size > 1000 and abs(ratios.mean()) < 0.1 and 0.9 < ratios.std() < 1.1, (ratios.size, ratios.mean(), ratios.std())


# ---- the composition itself --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bias, relu, residual", list(fs.EPILOGUE.values()), ids=list(fs.EPILOGUE))
def test_composition_against_autograd(bias, relu, residual):
    rs = np.random.RandomState(3)
    N, F, H, W = 2, 3, 4, 5
    s, b, r, dy = rs.randn(N, F, H, W), rs.randn(F), rs.randn(N, F, H, W), rs.randn(N, F, H, W)
    s[0, 0, 0, :2] = (0.0, -0.0)                # (with a ReLU alone: z exactly zero, which y <= 0 cuts as autograd does)
    ts, tb, tr = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (s, b, r))
    z = ts
    if bias: z = z + tb.view(1, -1, 1, 1)
    if residual: z = z + tr
    y = torch.relu(z) if relu else z
    y.backward(torch.tensor(dy))
    want_y = fs.compose(s, b if bias else None, r if residual else None, bool(relu))
    assert np.array_equal(want_y, y.detach().numpy())
    dz, dbias = fs.epilogue_grads(dy, want_y, bool(relu))
    assert np.array_equal(dz, ts.grad.numpy())                      # the gradient of the sum ...
    if residual:
        assert np.array_equal(dz, tr.grad.numpy())                  # ... is the residual's
    if bias:
        np.testing.assert_allclose(dbias, tb.grad.numpy(), rtol=1e-13, atol=1e-13)
    if relu:
        assert 0.2 < float((dz == 0).mean()) < 0.8
    # the bound on dbias is test_gpu_epilogue._check_dbias's
    assert np.array_equal(fs.dbias_bound(dz), 2.0 ** -16 * np.abs(dz).sum(axis=(0, 2, 3)))


def test_input_mask_against_autograd():
    rs = np.random.RandomState(4)
    x, g = rs.randn(2, 3, 4, 5), rs.randn(2, 3, 4, 5)
    x[0, 0, 0, :3] = (0.0, -0.0, -np.inf)
    tx = torch.tensor(x, requires_grad=True)
    y = torch.relu(tx)
    y.backward(torch.tensor(g))
    assert np.array_equal(fs.clamp_input(x), y.detach().numpy()) and not np.signbit(fs.clamp_input(x)[0, 0, 0, 1])
    assert np.array_equal(fs.mask_dx(x, g), tx.grad.numpy())
    assert 0.2 < float((fs.mask_dx(x, g) == 0).mean()) < 0.8


def test_reference_composes_the_pieces():
    """reference() on a seed with everything on: its tensors are the pieces applied to the oracle's, in the order of the issue"""
    from oracle import dau_oracle as orc
    seed = next(s for s in SEEDS if fs.config(s)["epilogue"] == "bias+relu+residual" and fs.config(s)["input_relu"])
    cfg = fs.config(seed)
    inp = fs.inputs(cfg)
    ref = fs.reference(cfg, inp)
    kw = dict(ignore=cfg["ignore"], **cfg["flags"])
    xc = np.where(inp["x"] <= 0, np.float32(0), inp["x"])
    s = orc.forward(xc, inp["w"], inp["mu1"], inp["mu2"], cfg["sigma"], **kw)
    assert np.array_equal(ref["s"], s) and ref["bias"].shape == (cfg["F"],) and ref["r"].shape == s.shape
    assert np.array_equal(fs.rounded(ref["r"], cfg["storage"]), ref["r"])
    z = (s.astype(np.float64) + ref["bias"].astype(np.float64)[None, :, None, None]) + ref["r"]
    assert np.array_equal(ref["y"], np.maximum(z, 0))
    # a "stored y" that disagrees with y_ref in sign at some elements: the backward follows the stored one
    y_gpu = fs.rounded(ref["y"].astype(np.float32), cfg["storage"]).copy()
    y_gpu[0, 0, 0, :] = 0.0
    full = fs.reference(cfg, inp, y_gpu)
    dz = np.where(y_gpu <= 0, 0, inp["dy"])
    assert np.array_equal(full["dz"], dz) and np.allclose(full["dbias"], dz.astype(np.float64).sum(axis=(0, 2, 3)), rtol=1e-12, atol=1e-12)
    want = orc.backward(xc, dz, inp["w"], inp["mu1"], inp["mu2"], cfg["sigma"], unit_testing=cfg["unit_testing"],
                        mu_learning_rate_factor=fs.LR, **kw)
    for key in fs.GRADS:
        assert np.array_equal(full[key], want[key]), key
    assert np.array_equal(full["dx"], np.where(inp["x"] <= 0, 0, want["dx"])) and bool((full["dx"][inp["x"] <= 0] == 0).all())
