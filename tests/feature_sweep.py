"""Seeded random shapes through the fused, 16-bit and NHWC paths TOGETHER (helper module of test_feature_sweep_plan.py and
test_gpu_feature_sweep.py; not a test, and nothing here touches a device or loads the HIP library).

config(seed) is one configuration.  Shape, kernel size, sigma, offset range, reference flags and ignored units are drawn as
test_gpu_fuzz._config draws them (from a stream of its own: other shapes than the fuzz's); the FEATURES -- storage format, layout,
members, input ReLU, epilogue of the second call -- are digits of the seed, not coin flips: storage = seed mod 3, the others the
mixed-radix digits (8, 4, 2, 2) of seed * STRIDE mod 128 with STRIDE odd, so 3 and 128 being coprime every 384 consecutive seeds hold
every combination once, and that the first 96 hold every PAIR of values of two features at least twice is a property of the table
that test_feature_sweep_plan.py asserts.

What the generator enforces beyond the fuzz's draws:
  * seeds that name DAU_FLAG_DENSE_SPLIT_F16 (members "split", "outliers"): sigma <= 1.0 (prefilter supports up to 11 taps have a
    staging instantiation) and an offset range within +-4, the clip and the bucket radius being those of the dense members (3.99
    and 4) whatever the plan's kernel size -- as the split sweep of test_gpu_fuzz.py does, so that the call runs the members the seed
    names; the default and NO_DENSE_SPLIT seeds keep the whole range of their kernel size;
  * "outliers" seeds: interpolation on, offsets within +-3 (a pin at the clip is exactly 3.0, which is no outlier), exactly one live
    unit moved to 3.5, and at least 100 live units (the member takes calls with at most 1 % of them beyond +-3);
  * seeds whose epilogue has a ReLU have at least three output channels: with one or two the sign of a channel's mean decides what
    the ReLU cuts, all or nothing (F = 1 and 2 stay with the other epilogues);
  * every fifth seed that names no dense member is a kernel-65, nine-unit plan with an offset range beyond +-24: the plans whose
    gather-sum pass takes four offset windows (1 % of the fuzz's draws), in the hinted call too;
  * units 0 and 1 are pinned to (+c, -c) and (-c, +c), c by cfg["c_mode"]: the drawn range, an integer inside it, the clip
    k // 2 - 0.01, or -- a quarter of the non-outlier seeds -- exactly the radius R of the smallest bucket that covers the range.
    Exactly R is legal (dau_conv_check_status reports max|mu| > bucket only); its +R+1 tap has weight 0.

inputs(cfg) draws the tensors, reference(cfg, inputs, y_gpu) composes the expected ones in float64 on top of oracle.dau_oracle:
    x' = where(x <= 0, 0, x) | x;  s = forward(x');  z = (s + bias) + r;  y = max(z, 0) | z
    dz = where(y_gpu <= 0, 0, dy) | dy;  dbias = sum dz;  backward(x', dz);  dx masked by x <= 0
(the backward from the GPU's STORED y: that is the ABI's contract).  The pieces of that composition are functions of their own
(clamp_input, compose, epilogue_grads, mask_dx), which test_feature_sweep_plan.py holds against torch's autograd."""
import math
from collections import OrderedDict

import numpy as np

DEFAULT_SEEDS = 96

# include/dau_conv.h (test_feature_sweep_plan.py holds these against dau_conv._capi)
FLAG_USE_INTERPOLATION, FLAG_UNIT_TESTING, FLAG_SINGLE_DIM_KERNEL, FLAG_FORBID_POSITIVE_DIM1 = 1 << 0, 1 << 1, 1 << 2, 1 << 3
FLAG_IO_BF16, FLAG_IO_F16, FLAG_IO_NHWC, FLAG_INPUT_RELU = 1 << 4, 1 << 11, 1 << 13, 1 << 14
FLAG_DENSE_SPLIT_F16, FLAG_NO_DENSE_SPLIT, FLAG_DENSE_SPLIT_OUTLIERS = 1 << 9, 1 << 10, 1 << 12
EPILOGUE_BIAS, EPILOGUE_RELU = 1, 2

STORAGE = ("f32", "f16", "bf16")
LAYOUT = ("nchw", "nhwc")
MEMBERS = ("default", "exact", "split", "outliers")
INPUT_RELU = (False, True)
# (bias, relu, residual) of the second forward call
EPILOGUE = OrderedDict((("none", (0, 0, 0)), ("bias", (1, 0, 0)), ("bias+relu", (1, 1, 0)), ("relu", (0, 1, 0)),
                        ("residual", (0, 0, 1)), ("bias+residual", (1, 0, 1)), ("bias+relu+residual", (1, 1, 1)),
                        ("relu+residual", (0, 1, 1))))
FEATURES = OrderedDict((("storage", STORAGE), ("layout", LAYOUT), ("members", MEMBERS), ("input_relu", INPUT_RELU),
                        ("epilogue", tuple(EPILOGUE))))
STRIDE = 37                       # odd: seed -> seed * STRIDE mod 128 is a bijection
RNG_BASE = 22940                  # of the shape draws: a stream of its own, chosen once so that the table covers what
                                  # test_feature_sweep_plan.py lists (pins at R = 8, default plans with the split gather-dot)
WINDOW_EVERY = 5
RELU_MIN_F = 3                    # output channels of a seed whose epilogue has a ReLU
IOFLAG = {"f32": 0, "f16": FLAG_IO_F16, "bf16": FLAG_IO_BF16}
MEMBER_FLAGS = {"default": 0, "exact": FLAG_NO_DENSE_SPLIT, "split": FLAG_DENSE_SPLIT_F16,
                "outliers": FLAG_DENSE_SPLIT_F16 | FLAG_DENSE_SPLIT_OUTLIERS}
C_MODES = ("range", "integer", "clip", "bucket")
BUCKETS = (4, 8, 16, 18, 20, 24, 32)
MIN_OUTLIER_UNITS = 100           # 1 % of the live units, rounded down, must leave room for the one outlier
OUTLIER_OFFSET = 3.5
LR = 10.0                         # mu_learning_rate_factor, as the fuzz uses
# (rel, floor) of util.assert_parity for y and dx: its defaults; tests/test_gpu_f16.py; tests/test_gpu_bf16.py
BARS = {"f32": (1e-4, 1e-6), "f16": (2e-3, 1e-3), "bf16": (2e-2, 4e-3)}
GRADS = ("dw", "dmu1", "dmu2", "dsigma")


def features(seed):
    """the covering enumeration: {feature: value} of a seed"""
    u = seed * STRIDE % 128
    return OrderedDict((("storage", STORAGE[seed % 3]), ("layout", LAYOUT[u // 64 % 2]), ("members", MEMBERS[u // 8 % 4]),
                        ("input_relu", INPUT_RELU[u // 32 % 2]), ("epilogue", tuple(EPILOGUE)[u % 8])))


def bucket_of(m):
    """the radius of the smallest offset bucket that covers +-m"""
    return next(b for b in BUCKETS if m <= b)


def config(seed):
    ft = features(seed)
    dense = ft["members"] in ("split", "outliers")
    outliers = ft["members"] == "outliers"
    # the kernel-65, nine-unit plans are the ones whose gather-sum takes four offset windows: every fifth seed that names no dense
    # member is one, with an offset range beyond +-24, so that the hinted call takes the windows too (1 % of the fuzz's draws are)
    windows = seed % WINDOW_EVERY == WINDOW_EVERY - 1 and not dense
    # ---- the draws of test_gpu_fuzz._config, in its order
    rs = np.random.RandomState(RNG_BASE + seed)
    k = int(rs.choice([9, 9, 9, 17, 17, 33, 65, 37, 41, 49]))
    H = int(rs.randint(5, 80)); W = int(rs.randint(5, 80))
    if seed % 7 == 0:
        H, W = int(rs.choice([56, 64, 96, 112])), int(rs.choice([56, 64, 72, 120]))
    G = int(rs.choice([1, 2, 2, 3, 4, 4, 5, 6, 8, 9]))
    if windows:
        k, G = 65, 9
    budget = 6.0e6 / (H * W * G)          # keep the oracle's work bounded
    S = int(rs.randint(1, 41))
    F = int(rs.randint(1, 71))
    N = int(rs.randint(1, 6))
    flags = dict(use_interpolation=bool(rs.rand() > 0.15), single_dim_kernel=bool(rs.rand() < 0.15),
                 forbid_positive_dim1=bool(rs.rand() < 0.15))
    unit_testing = bool(rs.rand() < 0.5)
    ignore = int(rs.randint(0, G)) if rs.rand() < 0.25 else 0
    sigma = float(rs.choice([0.5, 0.5, 0.5, 0.3, 0.8, 1.0, 1.4]))
    m = float(rs.uniform(0.5, k // 2))
    c_mode = C_MODES[int(rs.randint(4))]
    # ---- what the features ask of them
    if windows:
        m = 24.0 + m / 4.0
    while N * S * F > budget and (S > 1 or F > 1 or N > 1):
        if N > 1: N -= 1
        elif S >= F: S = max(1, S // 2)
        else: F = max(1, F // 2)
    if EPILOGUE[ft["epilogue"]][1]:
        F = max(F, RELU_MIN_F)
    if outliers:
        flags["use_interpolation"] = True
        while S * F * (G - ignore) < MIN_OUTLIER_UNITS:
            if ignore: ignore -= 1
            elif N > 1: N -= 1
            elif F <= S: F += 1
            else: S += 1
    if dense and sigma > 1.0:
        sigma = 0.5
    lim = k // 2 - 0.01                       # the layer's clip
    if dense:
        m, lim = min(m, 4.0), 3.99
    if outliers:
        m, lim = min(m, 3.0), 3.0
        if c_mode == "bucket":
            c_mode = "range"
    c = {"range": min(m, lim), "integer": float(math.floor(min(m, lim))), "clip": lim, "bucket": float(bucket_of(m))}[c_mode]
    bias, relu, residual = (bool(b) for b in EPILOGUE[ft["epilogue"]])
    return dict(seed=seed, N=N, S=S, F=F, G=G, H=H, W=W, k=k, flags=flags, unit_testing=unit_testing, ignore=ignore, sigma=sigma,
                m=m, lim=lim, c_mode=c_mode, c=float(c), storage=ft["storage"], nhwc=ft["layout"] == "nhwc", members=ft["members"],
                input_relu=ft["input_relu"], epilogue=ft["epilogue"], bias=bias, relu=relu, residual=residual)


def plan_flags(cfg):
    fl = IOFLAG[cfg["storage"]] | MEMBER_FLAGS[cfg["members"]]
    if cfg["flags"]["use_interpolation"]: fl |= FLAG_USE_INTERPOLATION
    if cfg["flags"]["single_dim_kernel"]: fl |= FLAG_SINGLE_DIM_KERNEL
    if cfg["flags"]["forbid_positive_dim1"]: fl |= FLAG_FORBID_POSITIVE_DIM1
    if cfg["unit_testing"]: fl |= FLAG_UNIT_TESTING
    if cfg["nhwc"]: fl |= FLAG_IO_NHWC
    if cfg["input_relu"]: fl |= FLAG_INPUT_RELU
    return fl


def plan_kwargs(cfg):
    """the keyword arguments of dau_conv._capi.Plan after (N, S, F, G, H, W)"""
    return dict(max_kernel_size=cfg["k"], number_units_ignore=cfg["ignore"], flags=plan_flags(cfg), sigma_hint=cfg["sigma"],
                mu_learning_rate_factor=LR)


def shape(cfg):
    return tuple(cfg[q] for q in ("N", "S", "F", "G", "H", "W"))


def epilogue_bits(cfg):
    return (EPILOGUE_BIAS if cfg["bias"] else 0) | (EPILOGUE_RELU if cfg["relu"] else 0)


def has_epilogue(cfg):
    return cfg["bias"] or cfg["relu"] or cfg["residual"]


def tag(cfg):
    """storage format and feature tuple, for names and messages"""
    return "seed%02d/%s/%s/%s/%s/%s" % (cfg["seed"], cfg["storage"], "nhwc" if cfg["nhwc"] else "nchw", cfg["members"],
                                         "inrelu" if cfg["input_relu"] else "raw", cfg["epilogue"])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

def rounded(a, storage):
    """float32 array -> the float32 values its storage format holds"""
    if storage == "f32":
        return a
    import torch
    return torch.from_numpy(a).to({"f16": torch.float16, "bf16": torch.bfloat16}[storage]).float().numpy()


def inputs(cfg):
    """-> dict of x, dy (float32 values of the storage format: what the kernels read), w, mu1, mu2 (float32)"""
    N, S, F, G, H, W = shape(cfg)
    rs = np.random.RandomState(33000 + cfg["seed"])
    # sign-symmetric where the input ReLU is on, so that it cuts about half
    x = (rs.randn(N, S, H, W) if cfg["input_relu"] else rs.rand(N, S, H, W)).astype(np.float32)
    dy = rs.randn(N, F, H, W).astype(np.float32)
    w = (rs.randn(1, S, G, F) * 0.1).astype(np.float32)
    m, lim, c = cfg["m"], cfg["lim"], cfg["c"]
    mu1 = np.clip(rs.uniform(-m, m, (1, S, G, F)), -lim, lim).astype(np.float32)
    mu2 = np.clip(rs.uniform(-m, m, (1, S, G, F)), -lim, lim).astype(np.float32)
    mu1.flat[0], mu2.flat[0] = c, -c
    if mu1.size > 1:
        mu1.flat[1], mu2.flat[1] = -c, c
    if cfg["members"] == "outliers":
        g = np.arange(mu1.size) // F % G
        live = np.flatnonzero((g < G - cfg["ignore"]) & (np.arange(mu1.size) >= 2))
        mu1.flat[live[rs.randint(len(live))]] = OUTLIER_OFFSET
    if cfg["flags"]["single_dim_kernel"]:
        mu2[:] = 0.0
    return dict(x=rounded(x, cfg["storage"]), dy=rounded(dy, cfg["storage"]), w=w, mu1=mu1, mu2=mu2)


def outlier_units(cfg, inp):
    """the live units with max(|mu1|, |mu2|) > 3: what dau_conv_gather_outlier_status counts"""
    G = cfg["G"]
    return int((np.maximum(np.abs(inp["mu1"]), np.abs(inp["mu2"]))[:, :, :G - cfg["ignore"], :] > 3).sum())


# ---- the composition, piece by piece (float64 numpy) ------------------------------------------------------------------------------

def clamp_input(x):
    """the input ReLU: a NaN stays, -0 becomes +0"""
    return np.where(x <= 0, np.zeros_like(x), x)


def mask_dx(x, dx):
    """its backward: the gradient passes where x > 0"""
    return np.where(x <= 0, np.zeros_like(dx), dx)


def compose(s, bias=None, r=None, relu=False):
    """y = act((s + bias[f]) + r): the adds in that order"""
    z = np.asarray(s, np.float64)
    if bias is not None:
        z = z + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
    if r is not None:
        z = z + np.asarray(r, np.float64)
    return np.maximum(z, 0.0) if relu else z


def epilogue_grads(dy, y, relu):
    """-> (dz, dbias): dz = where(y <= 0, 0, dy) from the STORED y (dy itself without a ReLU) -- the gradient of the sum and of the
    residual alike; dbias = dz summed over n, h, w in float64"""
    dy = np.asarray(dy, np.float64)
    dz = np.where(np.asarray(y) <= 0, 0.0, dy) if relu else dy
    return dz, dz.sum(axis=(0, 2, 3))


def dbias_bound(dz):
    """test_gpu_epilogue._check_dbias's: no value passes through more than 256 fp32 additions"""
    return 2.0 ** -16 * np.abs(np.asarray(dz, np.float64)).sum(axis=(0, 2, 3))


# ---- the reference --------------------------------------------------------------------------------------------------------------

def _oracle_kw(cfg):
    return dict(ignore=cfg["ignore"], **cfg["flags"])


POWER = 100.0                     # a forgotten term moves y_ref by more than this many bars at the max-norm (floor * max|y_ref|)
BIAS_DRAWS = 1000                 # at most; float32 and float16 seeds take their first


def power(cfg, s, bias, r, y=None):
    """-> {term: max|y_ref without the term - y_ref| in bars at the max-norm (floor * max|y_ref|) of the storage format}"""
    y = compose(s, bias, r, cfg["relu"]) if y is None else y
    bar = BARS[cfg["storage"]][1] * np.abs(y).max()
    out = {}
    if bias is not None:
        out["bias"] = float(np.abs(compose(s, None, r, cfg["relu"]) - y).max() / bar)
    if r is not None:
        out["residual"] = float(np.abs(compose(s, bias, None, cfg["relu"]) - y).max() / bar)
    return out


def _bias_power_by_channel(cfg, hi, lo, b):
    """power(...)["bias"] from the per-channel extremes of s + r alone (the adds in another order: equal but for float64 rounding)"""
    if cfg["relu"]:
        top = np.maximum(hi + b, 0.0).max()
        moved = np.where(b > 0, np.minimum(b, hi + b), np.minimum(-b, hi)).max()
    else:
        top = np.maximum(np.abs(hi + b), np.abs(lo + b)).max()
        moved = np.abs(b).max()
    return moved / (BARS[cfg["storage"]][1] * top) if top > 0 else 0.0


def forward_terms(cfg, inp):
    """-> dict of xc (the clamped x), s (the plain forward), bias [F] float32 or None, r (as stored) or None, y (float64).

    Bias and residual are drawn after s is known, at its size, so that a ReLU cuts about half of z and the max-norm floor of the bar
    keeps its meaning.  The bias is N(0, std(s)^2) per channel CONDITIONED on what test_feature_sweep_plan.py asserts of the inputs:
    the seed's stream is drawn on until leaving the bias (and the residual) out moves y_ref by more than POWER bars at the max-norm
    and a ReLU still cuts between 0.2 and 0.8.  Every float32 and float16 seed takes its first draw.  bfloat16's bar is 4e-3 of
    max|y_ref|, and beside a residual max|y_ref| is about |bias| + 3.5 std(s) in the bias's own channel: the draw that passes has a
    channel beyond some 2.3 standard deviations, two to twelve draws on in the default seeds."""
    from oracle import dau_oracle as orc
    xc = clamp_input(inp["x"]) if cfg["input_relu"] else inp["x"]
    s = orc.forward(xc, inp["w"], inp["mu1"], inp["mu2"], cfg["sigma"], **_oracle_kw(cfg))
    rs = np.random.RandomState(35000 + cfg["seed"])
    std = float(np.asarray(s, np.float64).std())
    draw_bias = lambda: (rs.randn(cfg["F"]) * std).astype(np.float32)
    bias = draw_bias() if cfg["bias"] else None
    r = rounded((rs.randn(*s.shape) * std).astype(np.float32), cfg["storage"]) if cfg["residual"] else None
    draws = 1 if cfg["bias"] else 0
    if cfg["bias"]:
        base = compose(s, None, r, False)
        hi, lo = base.max(axis=(0, 2, 3)), base.min(axis=(0, 2, 3))
        while draws < BIAS_DRAWS:
            if _bias_power_by_channel(cfg, hi, lo, bias.astype(np.float64)) > POWER:
                y = compose(s, bias, r, cfg["relu"])
                if min(power(cfg, s, bias, r, y).values()) > POWER and (not cfg["relu"] or 0.2 < float((y <= 0).mean()) < 0.8):
                    break
            bias = draw_bias()
            draws += 1
    return dict(xc=xc, s=s, bias=bias, r=r, y=compose(s, bias, r, cfg["relu"]), bias_draws=draws)


def reference(cfg, inp, y_gpu=None, terms=None):
    """The expected tensors.  Without y_gpu: the forward ones (forward_terms).  With y_gpu -- the second call's stored y, widened,
    logical [N, F, H, W] -- also dz, dbias and the five gradients of backward(x', dz), dx masked where the input ReLU is on."""
    from oracle import dau_oracle as orc
    out = dict(terms if terms is not None else forward_terms(cfg, inp))
    if y_gpu is None:
        return out
    dz, dbias = epilogue_grads(inp["dy"], y_gpu, cfg["relu"])
    out["dz"], out["dbias"] = dz, dbias
    got = orc.backward(out["xc"], dz.astype(np.float32), inp["w"], inp["mu1"], inp["mu2"], cfg["sigma"],
                       unit_testing=cfg["unit_testing"], mu_learning_rate_factor=LR, **_oracle_kw(cfg))
    if cfg["input_relu"]:
        got["dx"] = mask_dx(inp["x"], got["dx"])
    out.update(got)
    return out
