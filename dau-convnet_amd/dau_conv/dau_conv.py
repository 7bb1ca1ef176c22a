"""Python surface of the DAU convolution operator, PyTorch-ROCm binding.

Mirrors plugins/tensorflow/dau_conv/dau_conv.py of the reference (same class / function /
argument / variable names and defaults) on top of the C ABI in include/dau_conv.h:

    reference                                   here
    ------------------------------------------  -------------------------------------------
    dau_conv_op_module.dau_conv  (:212-219)     dau_conv(...)        raw op, TF attr names
    dau_conv_grad_module.dau_conv_grad          dau_conv_grad(...)   raw grad op
      (_dau_conv_grad_op.py:40-60)
    @ops.RegisterGradient("DAUConv") (:14)      _DAUConvFunction (torch.autograd.Function); under torch.compile the op
                                                torch.ops.dau_conv.conv (_ops.py).  Both run the one core, _forward / _backward
                                                below (layouts, offset checks, the plan's passes); what a plan does not fuse,
                                                eager applies in torch around the function, the op inside itself
    DAUGridMean (:24-74), ZeroNLast (:76-110)   same names (initializers)
    _DAUConvolution2d (:113-219)                same name
    DAUConv2d (:221-555), DAUConv1d (:557-570)  same names (torch.nn.Module)
    dau_conv2d (:580-690), dau_conv1d (:692-795) same names (scope-keyed functional form)

Parameters keep the reference's names and shapes: `weights`, `mu1`, `mu2` [1,S,G,F],
`sigma` (1,), `bias` (F,)  (dau_conv.py:389-440), so checkpoints map one to one.
There is no CPU / eager fallback: every call goes through libdau_conv_hip.so.
"""
import collections
import math
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import _capi

__all__ = ["DAUGridMean", "ZeroNLast", "DAUConv2d", "DAUConv1d", "dau_conv2d", "dau_conv1d", "dau_conv",
           "dau_conv_grad", "check_pending_offsets", "is_channels_last", "release_captured_plans"]


# ----------------------------------------------------------------------------------------------
# raw ops (attr names and defaults of REGISTER_OP("DAUConv") / ("DAUConvGrad"),
# plugins/tensorflow/src/dau_conv_op.cpp:22-48, dau_conv_grad_op.cpp:18-49)
# ----------------------------------------------------------------------------------------------
# Plans are cached per (shape, attrs, prefilter support, device) in least-recently-used order.  sigma enters a plan only
# through the prefilter support 2*ceil(5*sigma)+1 (the taps come from the device tensor on every call), so the key holds that
# number, not sigma: a trainable sigma changes every optimizer step and must keep hitting the same plan -- its kernel sets, its
# offset-bucket hint and its pending status.  The cache is bounded; a dropped plan is asked for its status first.
_PLANS = collections.OrderedDict()
_PLAN_CACHE_MAX = 64
# The keys of the plans a call has used while its stream was being captured into a graph (torch.cuda.graph, make_graphed_callables,
# the cudagraph trees of torch.compile).  Every replay of such a graph writes the plan's pinned status mirror, which dies with the
# plan: these plans stay in _PLANS, the eviction skips them and they do not count against _PLAN_CACHE_MAX, until
# release_captured_plans().
_PINNED = set()


def _pin(plan):
    """A captured call has used this plan: keep it (a plan made outside the cache has no key and is its caller's to keep)."""
    key = getattr(plan, "_cache_key", None)
    if key is not None and _PLANS.get(key) is plan:
        _PINNED.add(key)


def _evict():
    """Drop the least recently used plans that no captured graph uses until the others number _PLAN_CACHE_MAX at most."""
    if _PINNED:
        _PINNED.intersection_update(_PLANS.keys())   # (a cache that was emptied by hand takes its pins with it)
    while len(_PLANS) - len(_PINNED) > _PLAN_CACHE_MAX:
        key = next(iter(_PLANS)) if not _PINNED else next(k for k in _PLANS if k not in _PINNED)
        old = _PLANS.pop(key)
        old.last_status()        # a NaN / out-of-range offset it has seen and not yet reported is raised here, not lost


def release_captured_plans():
    """For a caller who has deleted their graphs: the plans that captured calls have used are ordinary cache entries again (and the
    oldest are dropped if the cache is over its bound).  A graph that is replayed after this may write the freed status mirror of a
    dropped plan: call it only when no such graph is left."""
    _PINNED.clear()
    _evict()


def is_channels_last(t):
    """True for a rank-4 tensor laid out [N][H][W][C] in memory (torch.channels_last) and not also NCHW-contiguous: tensors
    whose strides fit both (C = 1, or H = W = 1) count as contiguous."""
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


# channels_last=None: does a channels_last input of this dtype run the NHWC plan?  Decided by measurement: the
# NHWC plan against what a channels_last model pays around the NCHW plan -- x.contiguous(), y -> channels_last, dy.contiguous(),
# dx -> channels_last -- at the north-star layer: 23.66 against 25.66 ms (float32), 23.03 against 24.46 (float16), 21.18 against
# 22.53 (bfloat16), the rounds of one box within 0.1 ms of each other.  channels_last=True runs the NHWC plan whatever this table says.
_NHWC_BY_DEFAULT = {torch.float32: True, torch.float16: True, torch.bfloat16: True}


def _wants_nhwc(x, settings):
    """Should this call run an NHWC plan, as far as the input and the settings go (the library may still refuse the shape)."""
    cl = settings["channels_last"]
    if cl is False or not is_channels_last(x):
        return False
    if x.dtype == torch.bfloat16 and settings["dense_bf16"]:
        return False                     # DAU_FLAG_IO_NHWC excludes DAU_FLAG_DENSE_BF16: that layer converts, as before
    return True if cl is True else _NHWC_BY_DEFAULT.get(x.dtype, False)


def _check_activations(activation, input_activation):
    for prefix, value in (("", activation), ("input_", input_activation)):
        if value not in (None, "relu"):
            raise _capi.InvalidArgumentError(prefix + "activation must be None or \"relu\"")


def _check_weights(x, w, settings):
    if w.shape[1] != x.shape[1]:
        raise _capi.InvalidArgumentError("weights dim 1 (%d) must equal the input channels (%d)" % (w.shape[1], x.shape[1]))
    if w.shape[-1] != settings["num_output"]:
        # shape function of the op: last dim of every parameter == num_output (dau_conv_op.cpp:62-76)
        raise _capi.InvalidArgumentError("last dim of weights (%d) must equal num_output (%d)" % (w.shape[-1], settings["num_output"]))
    if settings["stride"] != 1:
        raise _capi.InvalidArgumentError("DAUConv: only stride=1 is supported")  # base_dau_conv_layer.cpp:68-69


def _check_bias(bias, w):
    if bias is not None and tuple(bias.shape) != (w.shape[-1],):
        raise _capi.InvalidArgumentError("bias has shape %s, expected (%d,)" % (tuple(bias.shape), w.shape[-1]))


def _residual_fusable(residual, x, w):
    """A residual the store can add: the input's dtype and exactly the output's shape (any other is added in torch)."""
    return residual.dtype == x.dtype and tuple(residual.shape) == (x.shape[0], w.shape[-1]) + tuple(x.shape[2:])


def _plan_flags(dtype, settings):
    """The DAU_FLAG_* bits of a call's plan, from its activation dtype and its settings; the optional flags are _get_plan's."""
    flags = 0
    if settings["use_interpolation"]:
        flags |= _capi.FLAG_USE_INTERPOLATION
    if settings["unit_testing"]:
        flags |= _capi.FLAG_UNIT_TESTING
    if settings["single_dim_kernel"]:
        flags |= _capi.FLAG_SINGLE_DIM_KERNEL
    if settings["forbid_positive_dim1"]:
        flags |= _capi.FLAG_FORBID_POSITIVE_DIM1
    if dtype == torch.bfloat16:
        flags |= _capi.FLAG_IO_BF16      # bfloat16 activations (input, output and their gradients); fp32 parameters
        if settings["dense_bf16"]:
            # calls whose offsets lie within +-4: the gather-sum passes (and, from three units on, the parameter gradients)
            # as densified bf16 MFMA GEMMs
            flags |= _capi.FLAG_DENSE_BF16
    elif dtype == torch.float16:
        # float16 activations (autocast, .half()): the members and the arithmetic of the fp32 plan, 16-bit loads and stores;
        # fp32 parameters.  dense_bf16 does not apply, as for fp32 input
        flags |= _capi.FLAG_IO_F16
    # the two-limb f16 dense gather-sum (fp32 accuracy): None = the library's choice (the radii that pay for this unit count)
    if settings["dense_split"] is True and not (flags & _capi.FLAG_DENSE_BF16):
        flags |= _capi.FLAG_DENSE_SPLIT_F16
    elif settings["dense_split"] is False:
        flags |= _capi.FLAG_NO_DENSE_SPLIT
    # opt-in: calls within +-4 with few units beyond +-3 keep the radius-3 dense GEMM, plus a ring pass over those units' outer taps
    if settings["dense_outliers"] and not (flags & (_capi.FLAG_DENSE_BF16 | _capi.FLAG_NO_DENSE_SPLIT)):
        flags |= _capi.FLAG_DENSE_SPLIT_OUTLIERS
    # opt-in, single-dimension layers: calls whose units lie on a line run the 1 x 9 / 1 x 17 two-limb GEMM (_settings has checked the
    # pairs: single-dimension, not dense_split=False, not dense_bf16)
    if settings["dense_line"]:
        flags |= _capi.FLAG_DENSE_SPLIT_LINE
    # likewise their parameter gradients: the line members of the two-limb gather-dot (the same pairs checked)
    if settings["dense_line_grads"]:
        flags |= _capi.FLAG_SPLIT_DOT_LINE
    return flags


_PlanKey = collections.namedtuple("_PlanKey", "N S F G H W kernel_size number_units_ignore flags algo support mu_learning_rate_factor device")


def _cached(key, make):
    """The plan cached under this _PlanKey, now the most recently used; else make(), stored under it."""
    plan = _PLANS.get(key)
    if plan is not None:
        _PLANS.move_to_end(key)
        return plan
    plan = make()
    if key.algo == _capi.ALGO_AUTO and _capi.ALGO_DIRECT in (plan.info["algo_forward"], plan.info["algo_backward"]):
        # the LDS-tiled kernels refused this shape (e.g. more than 16 units per channel pair under a kernel larger than 17, a
        # prefilter window or error row larger than the LDS): correct, but orders of magnitude slower -- say so once per plan
        which = [n for n, a in (("forward / input gradient", plan.info["algo_forward"]), ("parameter gradients", plan.info["algo_backward"]))
                 if a == _capi.ALGO_DIRECT]
        warnings.warn("DAUConv: N=%d C=%d->%d %dx%d, %d units, max_kernel_size=%d: the %s run on the plain one-thread-per-output "
                      "kernels (the tiled MFMA kernels do not support this shape); expect them to be orders of magnitude slower"
                      % (key.N, key.S, key.F, key.H, key.W, key.G, key.kernel_size, " and the ".join(which)), RuntimeWarning,
                      stacklevel=3)         # (the caller of _get_plan, which is the one caller of this)
    _PLANS[key] = plan
    plan._cache_key = key
    _evict()
    return plan


# Flags a call would like and the library may refuse for its shape (shapes that fall back to the direct kernels), outermost first, and
# the name by which its refusal tells which one it refuses.  _REFUSED: the plan keys that were refused so -- the flags outside the
# refused one decided, those inside it not yet set: each is asked once, then the call runs without the flag
_OPTIONAL_FLAGS = ((_capi.FLAG_INPUT_RELU, "DAU_FLAG_INPUT_RELU"), (_capi.FLAG_IO_NHWC, "DAU_FLAG_IO_NHWC"))
_REFUSED = set()


def _get_plan(x, w, settings, nhwc=False):
    """The cached plan of this call.  nhwc: the FLAG_IO_NHWC plan if the library builds one for the shape, else the NCHW plan
    (Plan.io_layout tells which came back).  settings["input_relu"]: the FLAG_INPUT_RELU plan where the library builds one, else
    the plan without the flag (Plan.input_relu tells which came back; the caller then applies the ReLU itself)."""
    N, S, H, W = x.shape
    _, _, G, F = w.shape
    _check_weights(x, w, settings)
    base = _plan_flags(x.dtype, settings)
    support, lr = _capi.filter_support(settings["sigma_hint"]), float(settings["mu_learning_rate_factor"])
    make_key = lambda fl: _PlanKey(N, S, F, G, H, W, settings["kernel_size"], settings["number_units_ignore"], fl, settings["algo"],
                                   support, lr, x.device.index)
    # (FLAG_INPUT_RELU excludes DAU_FLAG_DENSE_BF16: that layer applies the ReLU itself, unasked)
    wanted = (settings["input_relu"] and not base & _capi.FLAG_DENSE_BF16, nhwc)
    while True:
        flags, asked = base, []
        for (flag, name), want in zip(_OPTIONAL_FLAGS, wanted):
            if want and make_key(flags | flag) not in _REFUSED:
                flags |= flag
                asked.append((name, make_key(flags)))        # (what to remember if the library names this flag)
        try:
            return _cached(make_key(flags), lambda: _capi.Plan(
                N, S, F, G, H, W, max_kernel_size=settings["kernel_size"], number_units_ignore=settings["number_units_ignore"],
                flags=flags, algo=settings["algo"], sigma_hint=settings["sigma_hint"],
                mu_learning_rate_factor=settings["mu_learning_rate_factor"], device=x.device))
        except _capi.InvalidArgumentError as e:
            refused = [key for name, key in asked if name in str(e)]
            if not refused:
                raise
            _REFUSED.add(refused[-1])        # (the innermost flag named.)  No tiled kernels for this shape / algo: without it, as before


def _check_before(plan, mode):
    """check_offsets="async": before enqueueing a call, look at what the plan's most recent COMPLETED call reported
    (pinned host memory, no sync) and raise the reference's errors for it (NaN -> FailedPrecondition, offsets beyond the
    kernel -> InvalidArgument, dau_conv_op.cpp:250-262) -- one call late, without stalling the stream."""
    if mode == "async":
        plan.last_status()


def _check_after(plan, mode):
    """check_offsets=True: the reference's behaviour -- wait for the call and raise at once (the reference blocks on a
    D2H copy of the amax in every Compute, dau_conv_op.cpp:229-235)."""
    if mode is True:                                  # _settings normalises: "async", True or False, nothing else
        plan.check_status()


def check_pending_offsets(device=None):
    """Wait for the device and raise if any plan's latest call saw a NaN / out-of-range offset (for check_offsets="async"
    users: call at the end of a step or before reading results) -- or a sigma that needs a wider prefilter than the plan holds
    (FailedPreconditionError).  The second cannot happen to eager calls, which choose their plan from a fresh host copy of sigma; it
    is what a replayed graph must be asked for: its plans' supports are frozen at capture, no Python runs in a replay, and the device
    records what each call's sigma would have needed (Plan.sigma_status()).  A sigma that needs LESS than the plan holds is no
    error: the wider support is still a correct truncation.  Either record is reported once."""
    torch.cuda.synchronize(device)
    for plan in list(_PLANS.values()):
        plan.last_status()
    for plan in list(_PLANS.values()):
        _, planned, worst = plan.sigma_status()
        if worst > planned:
            raise _capi.FailedPreconditionError(
                "DAUConv: sigma has grown beyond the prefilter support of a captured plan: a call needed %d x %d taps "
                "(2*ceil(5*sigma)+1), the plan holds %d x %d (N=%d C=%d->%d %dx%d).  A replayed graph keeps the plan it was "
                "captured with: capture again" % (worst, worst, planned, planned, plan.N, plan.S, plan.F, plan.H, plan.W))


def _check_line_options(single_dim, dense_split, dense_bf16, dense_line, dense_line_grads):
    """The rules of the two opt-in line options, for the layer's constructor and for _settings() alike."""
    for option, on, flag in (("dense_line_grads", dense_line_grads, "DAU_FLAG_SPLIT_DOT_LINE"),
                             ("dense_line", dense_line, "DAU_FLAG_DENSE_SPLIT_LINE")):
        if on and not single_dim:
            raise ValueError("%s=True needs a single-dimension layer (DAUConv1d, or dau_unit_single_dim=True)" % option)
        if on and dense_split is not None and not dense_split:
            raise ValueError("%s=True excludes dense_split=False" % option)
        if on and dense_bf16:
            raise ValueError("%s=True excludes dense_bf16=True (%s excludes DAU_FLAG_DENSE_BF16)" % (option, flag))


def _settings(sigma, number_units_x=2, number_units_y=2, number_units_ignore=0, num_output=64, kernel_size=9, pad=4,
              stride=1, unit_normalization=True, square_unit_normalization=False, mean_iteration_step=1,
              sigma_iteration_step=1, component_border_bound=1.0, sigma_lower_bound=0.3, merge_iteration_step=0,
              merge_threshold=1, unit_testing=False, mu_learning_rate_factor=1.0, single_dim_kernel=False,
              forbid_positive_dim1=False, use_interpolation=True, sigma_hint=None, check_offsets="async",
              algo=_capi.ALGO_AUTO, dense_bf16=False, dense_split=None, process_group=None, grad_reduce="mean", name=None,
              dense_outliers=False, channels_last=None, dense_line=False, dense_line_grads=False):
    """The attrs of a call, checked and normalised: every key is always there (input_relu=False: the caller sets it for a call with
    the ReLU in front)."""
    _check_line_options(single_dim_kernel, dense_split, dense_bf16, dense_line, dense_line_grads)
    if not unit_normalization or square_unit_normalization:
        raise _capi.InvalidArgumentError("only unit_normalization=True, square_unit_normalization=False is implemented")
    if sigma_hint is None:
        # same host read of sigma[0] the reference performs in LayerSetUp (base_dau_conv_layer.cpp:140-143); under stream capture
        # the copy the last such read of this tensor left (_ops._sigma_hint)
        sigma_hint = _ops._sigma_hint(sigma, every_call=True)
    if grad_reduce not in ("mean", "sum"):
        raise _capi.InvalidArgumentError("grad_reduce must be \"mean\" or \"sum\"")
    # "async" or a truth value (1, 1.0, numpy.bool_ ... count as True): nothing else reaches _check_before / _check_after
    mode = "async" if (isinstance(check_offsets, str) and check_offsets == "async") else bool(check_offsets)
    return dict(number_units_ignore=int(number_units_ignore), num_output=int(num_output), kernel_size=int(kernel_size),
                stride=int(stride), unit_testing=bool(unit_testing), mu_learning_rate_factor=float(mu_learning_rate_factor),
                single_dim_kernel=bool(single_dim_kernel), forbid_positive_dim1=bool(forbid_positive_dim1),
                use_interpolation=bool(use_interpolation), sigma_hint=float(sigma_hint),
                check_offsets=mode, algo=int(algo), dense_bf16=bool(dense_bf16),
                dense_split=(None if dense_split is None else bool(dense_split)), dense_outliers=bool(dense_outliers),
                process_group=process_group, grad_reduce=grad_reduce,
                channels_last=(None if channels_last is None else bool(channels_last)), dense_line=bool(dense_line),
                dense_line_grads=bool(dense_line_grads), input_relu=False)


def _c(t):
    return t.contiguous() if not t.is_contiguous() else t


def _act(t, plan):
    """An activation in the layout the plan takes: channels_last for an NHWC plan, contiguous otherwise; copied only if it is not."""
    if plan.io_layout == "NHWC":
        return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)
    return _c(t)


def _f32(t):
    """A parameter of another floating dtype (model.half(), model.bfloat16()) as float32: differentiable, so autograd hands its
    gradient back in the parameter's own dtype; float32 tensors pass unchanged."""
    return t.float() if t.is_floating_point() and t.dtype != torch.float32 else t


def dau_conv_grad(grad, input, weights, mu1, mu2, sigma, need_mask=_capi.NEED_ALL, **attrs):
    """DAUConvGrad op -> (grad_input, grad_weights, grad_mu1, grad_mu2, grad_sigma).  The parameter gradients are float32."""
    attrs.setdefault("component_border_bound", 0.0)  # the only default that differs (dau_conv_grad_op.cpp:37)
    weights, mu1, mu2, sigma = _f32(weights), _f32(mu1), _f32(mu2), _f32(sigma)
    st = dict(_settings(sigma, **attrs), process_group=None)     # (the raw grad op is local: process_group= is the layer's)
    plan = _get_plan(input, weights, st, _wants_nhwc(input, st))
    return _backward(plan, st, _act(input, plan), grad, _c(weights), _c(mu1), _c(mu2), _c(sigma), need_mask)[2]


# The one forward / backward over a plan: eager (_DAUConvFunction, dau_conv_grad) and the torch.compile ops (_ops.conv,
# _ops.conv_backward) both run these two; what a caller adds is what its side alone needs (see each).
def _forward(plan, st, input, weights, mu1, mu2, sigma, bias=None, relu=False, residual=None):
    """-> (y, the input as the plan took it: what backward wants back).  bias / relu / residual: the epilogue fused into the store
    -- the caller has asked _epilogue_ok(plan); the parameters and the bias contiguous float32."""
    # a channels_last input runs the NHWC plan where there is one: no copy of x, y channels_last
    input = _act(input, plan)
    if residual is not None:
        residual = _act(residual, plan)
    mode = _check_mode(st, input)
    _check_before(plan, mode)
    y = plan.forward(input, weights, mu1, mu2, sigma, bias=bias, relu=relu, residual=residual)
    if plan.captured:
        _pin(plan)
    _check_after(plan, mode)
    return y, input


def _check_mode(st, input):
    """check_offsets of this call, and the refusals of a call under stream capture: check_offsets=True waits for the stream, which a
    capture cannot, and runs as "async" there; process_group= runs an all-reduce."""
    mode = st["check_offsets"]
    if (mode is True or st["process_group"] is not None) and _capi.capturing(input.device):
        if st["process_group"] is not None:
            raise _capi.InvalidArgumentError("DAUConv: a process_group= layer cannot be captured into a graph (its backward runs an "
                                             "all-reduce on a stream of its own); capture the layer without process_group=")
        return "async"
    return mode


def _need_mask(needs_input_grad):
    """The _capi.NEED_* bits of an autograd context whose first five inputs are (input, weights, mu1, mu2, sigma)."""
    bits = (_capi.NEED_DX, _capi.NEED_DW, _capi.NEED_DMU1, _capi.NEED_DMU2, _capi.NEED_DSIGMA)
    return sum(bit for bit, wanted in zip(bits, needs_input_grad) if wanted)


def _backward(plan, st, input, grad, weights, mu1, mu2, sigma, need, y=None, relu=False, need_dbias=False):
    """-> (the gradient of the sum, dbias, (dx, dw, dmu1, dmu2, dsigma)), for a caller that wants at least one of them.  input as
    _forward returned it; relu / need_dbias: backward of the fused epilogue, from the forward's y.  The residual joins the sum
    before the activation, so its gradient IS the first result (dz, or grad in the plan's layout without a ReLU)."""
    mode = _check_mode(st, input)
    _check_before(plan, mode)
    grad = _act(grad, plan)
    dbias = None
    if need_dbias or relu:
        # one pass: the gradient of the sum, dz = (y <= 0) ? 0 : grad, and the bias gradient (local: it is not exchanged)
        dz, dbias = plan.epilogue_backward(grad, _act(y, plan) if relu else None, relu=relu, need_dbias=need_dbias)
        if dz is not None:
            grad = dz
    if need == 0:
        return grad, dbias, (None,) * 5
    group = st["process_group"]
    if group is not None and need & ~_capi.NEED_DX and _group_size(group) > 1:
        out = _data_parallel_backward(plan, input, grad, weights, mu1, mu2, sigma, need, group, st["grad_reduce"])
    else:
        out = plan.backward(input, grad, weights, mu1, mu2, sigma, need)
    if plan.captured:
        _pin(plan)
    _check_after(plan, mode)
    return grad, dbias, out


class _DAUConvFunction(torch.autograd.Function):
    """Eager's caller of _forward / _backward; what the plan does not fuse, dau_conv() applies in torch around this function."""
    @staticmethod
    def forward(ctx, input, weights, mu1, mu2, sigma, st, bias=None, relu=False, residual=None):
        weights, mu1, mu2, sigma = _c(weights), _c(mu1), _c(mu2), _c(sigma)
        plan = _get_plan(input, weights, st, _wants_nhwc(input, st))
        y, input = _forward(plan, st, input, weights, mu1, mu2, sigma, None if bias is None else _c(bias), relu, residual)
        # (an input_relu plan: `input` is the raw tensor -- the ReLU's output is never materialised, nor saved); y for the ReLU mask
        ctx.save_for_backward(*((input, weights, mu1, mu2, sigma) + ((y,) if relu else ())))
        ctx.plan, ctx.st, ctx.relu = plan, st, bool(relu)
        return y

    @staticmethod
    def backward(ctx, grad):
        input, weights, mu1, mu2, sigma = ctx.saved_tensors[:5]
        y = ctx.saved_tensors[5] if ctx.relu else None
        need = _need_mask(ctx.needs_input_grad)
        n_in = len(ctx.needs_input_grad)             # 6, 8 with (bias, relu), 9 with the residual
        need_dbias = n_in > 6 and ctx.needs_input_grad[6]
        need_dres = n_in > 8 and ctx.needs_input_grad[8]
        if need == 0 and not need_dbias and not need_dres:
            return (None,) * n_in
        dsum, dbias, out = _backward(ctx.plan, ctx.st, input, grad, weights, mu1, mu2, sigma, need, y, ctx.relu, need_dbias)
        return (out + (None, dbias, None, dsum if need_dres else None))[:n_in]


def _group_size(group):
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size(None if group is True else group)


def _data_parallel_backward(plan, input, grad, weights, mu1, mu2, sigma, need, group, grad_reduce):
    """Backward of one batch shard in the order of SURVEY.md 8(e): raw parameter-gradient sums of the shard -> ONE asynchronous
    all-reduce of the flat [4, S, G, F] buffer -> the dx pass runs while the floats travel -> the elementwise tail
    (dmu *= w * lr, dsigma *= w, ignored units, NaN -> 0) on the REDUCED sums, so every rank ends bit-identical and a NaN on one
    rank reaches all of them.  grad_reduce="mean" divides the reduced sums by the group size (what DistributedDataParallel
    does to finalized gradients), "sum" leaves the sum over the global batch."""
    from .distributed import OverlappedBackward
    pg = None if group is True else group
    world = _group_size(group)
    ex = OverlappedBackward(weights.shape, input.device, group=pg)
    dx_fn = (lambda: plan.backward(input, grad, weights, mu1, mu2, sigma, _capi.NEED_DX)[0]) if need & _capi.NEED_DX else None

    def finalize(sums):
        if grad_reduce == "mean":
            sums.mul_(1.0 / world)
        return plan.finalize_param_grads(sums, weights, need_mask=need & ~_capi.NEED_DX)

    dx = ex.run(lambda out: plan.backward_param_sums(input, grad, mu1, mu2, sigma, out=out), dx_fn, finalize)
    return (dx,) + tuple(ex.wait())


def _epilogue_ok(plan):
    """Does the plan take the fused epilogue (asked once per plan)?"""
    ok = getattr(plan, "_epilogue_ok", None)
    if ok is None:
        try:
            ok = plan.epilogue_supported(_capi.EPILOGUE_BIAS | _capi.EPILOGUE_RELU)
        except _capi.InvalidArgumentError:
            ok = False                   # direct kernels, dense_bf16: the unfused form below
        plan._epilogue_ok = ok
    return ok


def _input_relu_ok(input, weights, sigma, attrs):
    """Does the plan of this call take the ReLU in front of it (FLAG_INPUT_RELU)?  Asked once per plan: _get_plan remembers a refusal.
    -> (answer, the sigma hint the settings were made with: read from the device at most once per call)"""
    st = dict(_settings(_f32(sigma), **attrs), input_relu=True)
    return _get_plan(input, _f32(weights), st, _wants_nhwc(input, st)).input_relu, st["sigma_hint"]


def dau_conv(input, weights, mu1, mu2, sigma, bias=None, activation=None, residual=None, input_activation=None, **attrs):
    """DAUConv op: output[n,f] = sum_{s,g} w * bilinear(blur_sigma(input[n,s]), . + (mu2, mu1)); differentiable.
    input (and so output) float32, bfloat16 or float16; the parameters are used as float32 whatever their floating dtype.
    bias ([F]) and activation (None or "relu"): output = act(output + bias[f]) fused into the kernels' store -- one fp32 add and a
    clamp before the one rounding, the output keeps the input's dtype, and backward takes the ReLU mask and the bias gradient (in
    the bias's dtype) in one pass.  Plans that have no fused epilogue (shapes on the direct kernels, dense_bf16) run the op, then
    `+ bias` and relu in torch, with torch's type promotion.
    residual (the shortcut of a residual block): output = act((output + bias[f]) + residual), the bias first.  A residual of the
    input's dtype and the output's shape is added inside the store as well -- in fp32, before the one rounding; it is brought to the
    plan's layout (copied only if needed), only read, and its gradient is the tensor backward hands the DAU passes (no extra pass).
    Any other residual (another dtype, a shape that broadcasts, a plan without the fused epilogue) is added in torch, with torch's
    promotion, after the op and its bias and before the activation.
    input_activation (None or "relu"): output = DAUConv(relu(input)) with the ReLU inside the op (conv -> BatchNorm -> ReLU -> DAU
    stacks pass the BatchNorm output): the kernels clamp the input where they load it and mask the input gradient by it in its store,
    so no ReLU pass runs forward or backward and autograd saves the raw input, not a ReLU output.  Bit for bit the results of
    dau_conv(torch.relu(input), ...).  Plans that cannot take it (shapes on the direct kernels, dense_bf16) apply torch.relu first.
    Under torch.compile (torch.compiler.is_compiling()) the call becomes the one opaque op torch.ops.dau_conv.conv (_ops.py), which
    makes these decisions at run time and reads sigma itself (a sigma_hint= is ignored there); process_group= calls leave the graph."""
    if torch.compiler.is_compiling():
        return _dau_conv_compiled(input, weights, mu1, mu2, sigma, bias, activation, residual, input_activation, attrs)
    _check_activations(activation, input_activation)
    if input_activation == "relu":
        ok, hint = _input_relu_ok(input, weights, sigma, attrs)
        attrs = dict(attrs, sigma_hint=hint)
        if not ok:
            return dau_conv(torch.relu(input), weights, mu1, mu2, sigma, bias=bias, activation=activation, residual=residual, **attrs)

    def residual_in_torch():
        out = dau_conv(input, weights, mu1, mu2, sigma, bias=bias, input_activation=input_activation, **attrs) + residual
        return torch.relu(out) if activation == "relu" else out
    if residual is not None and not _residual_fusable(residual, input, weights):
        return residual_in_torch()
    weights, mu1, mu2, sigma = _f32(weights), _f32(mu1), _f32(mu2), _f32(sigma)
    st = _settings(sigma, **attrs)
    st["input_relu"] = input_activation == "relu"        # part of the plan key (_get_plan): the plan takes the raw input
    if bias is None and activation is None and residual is None:
        return _DAUConvFunction.apply(input, weights, mu1, mu2, sigma, st)
    _check_bias(bias, weights)
    if _epilogue_ok(_get_plan(input, weights, st, _wants_nhwc(input, st))):
        args = (input, weights, mu1, mu2, sigma, st, None if bias is None else _f32(bias), activation == "relu")
        return _DAUConvFunction.apply(*(args if residual is None else args + (residual,)))
    if residual is not None:
        return residual_in_torch()
    out = _DAUConvFunction.apply(input, weights, mu1, mu2, sigma, st)
    if bias is not None:
        out = out + bias.reshape(1, -1, 1, 1)
    return torch.relu(out) if activation == "relu" else out


def _dau_conv_compiled(input, weights, mu1, mu2, sigma, bias, activation, residual, input_activation, attrs):
    """dau_conv() while Dynamo traces: everything decidable from arguments, dtypes and shapes here, the rest inside the op."""
    if attrs.get("process_group") is not None:
        # the overlapped all-reduce of _data_parallel_backward is not an op: today's function, outside the graph (one graph break)
        return _ops.process_group_eager()(dau_conv, input, weights, mu1, mu2, sigma, bias=bias, activation=activation,
                                          residual=residual, input_activation=input_activation, **attrs)
    _check_activations(activation, input_activation)
    if residual is not None and not _residual_fusable(residual, input, weights):
        out = _dau_conv_compiled(input, weights, mu1, mu2, sigma, bias, None, None, input_activation, attrs) + residual
        return torch.relu(out) if activation == "relu" else out
    st = _settings(sigma, **dict(attrs, sigma_hint=0.0))     # (a placeholder: sigma is not read while tracing)
    _check_weights(input, weights, st)
    _check_bias(bias, weights)
    return torch.ops.dau_conv.conv(input, weights, mu1, mu2, sigma, bias, residual, activation == "relu", input_activation == "relu",
                                   *_ops.encode_settings(st))


# ----------------------------------------------------------------------------------------------
# initializers
# ----------------------------------------------------------------------------------------------
class DAUGridMean(object):
    """Initializer placing the DAU offsets on a regular grid, equally spaced in each dimension.

    Args follow the reference (dau_conv.py:24-37): dau_units = units in each direction,
    max_value = limit of the unit positions from the centre, dau_unit_axis 2 => mu1, 1 => mu2.
    The value formula is the reference's (:50).  The reference then tiles with a list indexed
    by the unit COUNT (:61-62), which only produces a grid for some unit shapes; this
    implementation broadcasts along the requested axis, i.e. the documented intent
    (README.md:194-202).  `legacy_values()` returns the bare per-axis value vector.
    """

    def __init__(self, dau_units, max_value, dau_unit_axis=2):
        self.dau_units = tuple(int(u) for u in dau_units)
        self.dau_unit_axis = dau_unit_axis
        self.max_value = max_value

    def legacy_values(self, num_units):
        mv = self.max_value
        return np.arange(num_units) * (2 * mv + 1) / float(num_units) + (-0.5 + (2 * mv + 1) / float(2 * num_units)) - mv

    def __call__(self, shape, dtype=None, partition_info=None):
        assert len(shape) == 4, "DAUGridMean requires input of rank 4 with dims=[1, input_channels, mu1*mu2, out_filters]"
        shape = list(shape)
        separated = shape[2] != self.dau_units[0] * self.dau_units[1]
        if not separated:
            shape = [shape[1], self.dau_units[0], self.dau_units[1], shape[-1]]
        num_units = shape[self.dau_unit_axis]
        vals = self.legacy_values(num_units)
        view = [1, 1, 1, 1]
        view[self.dau_unit_axis] = num_units
        out = np.broadcast_to(vals.reshape(view), shape).astype(np.float32)
        if not separated:
            out = out.reshape(1, shape[0], shape[1] * shape[2], shape[3])
        return torch.from_numpy(np.ascontiguousarray(out))

    def get_config(self):
        return {"dau_units": self.dau_units, "dau_unit_axis": self.dau_unit_axis, "max_value": self.max_value}


class ZeroNLast(object):
    """Wrapper initializer that zeros the last N values along `axis` (dau_conv.py:76-110)."""

    def __init__(self, base_init, last_num_to_zero, axis):
        self.base_init = base_init
        self.last_num_to_zero = last_num_to_zero
        self.axis = axis

    def __call__(self, shape, dtype=None, partition_info=None):
        vals = _run_init(self.base_init, shape)
        idx = [slice(None)] * vals.dim()
        idx[self.axis] = slice(vals.shape[self.axis] - self.last_num_to_zero, None)
        vals[tuple(idx)] = 0
        return vals

    def get_config(self):
        return {"last_num_to_zero": self.last_num_to_zero, "axis": self.axis}


def random_normal_initializer(mean=0.0, stddev=1.0):
    return lambda shape, dtype=None, partition_info=None: torch.randn(*shape) * stddev + mean


def random_uniform_initializer(minval=0.0, maxval=1.0):
    return lambda shape, dtype=None, partition_info=None: torch.rand(*shape) * (maxval - minval) + minval


def constant_initializer(value=0.0):
    return lambda shape, dtype=None, partition_info=None: torch.full(tuple(shape), float(value))


def zeros_initializer():
    return constant_initializer(0.0)


def _run_init(init, shape):
    if torch.is_tensor(init):
        t = init.detach().clone().float()
    elif isinstance(init, (int, float)):
        t = torch.full(tuple(shape), float(init))
    else:
        t = init(tuple(shape))
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t)
        t = t.detach().clone().float()
    if tuple(t.shape) != tuple(shape):
        raise ValueError("initializer returned shape %s, expected %s" % (tuple(t.shape), tuple(shape)))
    return t


# ----------------------------------------------------------------------------------------------
# layer
# ----------------------------------------------------------------------------------------------
# The engine options: what this binding adds to the reference's layer arguments.  Each goes by one name as a DAUConv2d argument and
# attribute, a _DAUConvolution2d argument and attribute, and an attr of dau_conv()
_ENGINE_OPTIONS = ("check_offsets", "algo", "dense_bf16", "dense_split", "dense_outliers", "dense_line", "dense_line_grads",
                   "channels_last", "process_group", "grad_reduce")
# (attr of dau_conv(), the _DAUConvolution2d attribute it comes from)
_OP_ATTRS = (("num_output", "num_output"), ("number_units_ignore", "num_dau_units_ignore"), ("kernel_size", "max_kernel_size"),
             ("pad", "_pad"), ("component_border_bound", "dau_unit_border_bound"), ("sigma_lower_bound", "dau_unit_sigma_bound"),
             ("mu_learning_rate_factor", "mu_learning_rate_factor"), ("single_dim_kernel", "dau_unit_single_dim"),
             ("forbid_positive_dim1", "dau_aggregation_forbid_positive_dim1"), ("use_interpolation", "dau_mu_interpolation"),
             ("unit_testing", "unit_testing"), ("name", "name")) + tuple((option, option) for option in _ENGINE_OPTIONS)


class _DAUConvolution2d(object):
    """Helper that clips the offsets and calls the op (dau_conv.py:113-219)."""

    def __init__(self, input_shape, num_output, dau_units, max_kernel_size, padding, data_format=None, strides=None,
                 num_dau_units_ignore=0, mu_learning_rate_factor=500, dau_unit_border_bound=0.01,
                 dau_unit_sigma_bound=0.01, dau_unit_single_dim=False, dau_aggregation_forbid_positive_dim1=False,
                 dau_mu_interpolation=True, unit_testing=False, name=None, check_offsets="async", algo=_capi.ALGO_AUTO,
                 dense_bf16=False, process_group=None, grad_reduce="mean", dense_split=None, dense_outliers=False,
                 channels_last=None, dense_line=False, dense_line_grads=False):
        if len(input_shape) != 4:
            raise ValueError("Only two dimensional DAUConv supported (rank-4 NCHW input).")
        if data_format is None or data_format == "NHWC":
            raise ValueError("data_format \"NHWC\" not supported - TODO: manually convert to NHWC.")
        if data_format != "NCHW":
            raise ValueError("data_format must be \"NHWC\" or \"NCHW\".")
        if strides is None:
            strides = 1
        if strides > 1:
            raise ValueError("Only strides=1 supported.")
        self.num_output = num_output
        self.padding = padding
        self._pad = int(padding)         # (a Python int: a numpy scalar read while Dynamo traces would put an .item() into the graph)
        self.name = name
        self.dau_units = dau_units
        self.num_dau_units_ignore = num_dau_units_ignore
        self.max_kernel_size = max_kernel_size
        self.mu_learning_rate_factor = mu_learning_rate_factor
        self.dau_unit_border_bound = dau_unit_border_bound
        self.dau_unit_sigma_bound = dau_unit_sigma_bound
        self.dau_unit_single_dim = dau_unit_single_dim
        self.dau_aggregation_forbid_positive_dim1 = dau_aggregation_forbid_positive_dim1
        self.dau_mu_interpolation = dau_mu_interpolation
        self.unit_testing = unit_testing
        self.check_offsets = check_offsets
        self.algo = algo
        self.dense_bf16 = dense_bf16
        self.dense_split = dense_split
        self.dense_outliers = dense_outliers
        self.dense_line = dense_line
        self.dense_line_grads = dense_line_grads
        self.channels_last = channels_last
        self.process_group = process_group
        self.grad_reduce = grad_reduce
        if process_group is not None:
            _ops.process_group_eager()       # built here, not while Dynamo traces the first call
        self.mean_max_allowed_offset = float(np.floor(self.max_kernel_size / 2.0) - self.dau_unit_border_bound)

    def __call__(self, inp, w, mu1, mu2, sigma, sigma_hint=None, bias=None, activation=None, residual=None, input_activation=None):
        # clip in the graph, so clipped units receive zero mu-gradient (dau_conv.py:190-191)
        m = self.mean_max_allowed_offset
        mu1 = torch.clamp(mu1, min=-m, max=m)
        mu2 = torch.clamp(mu2, min=-m, max=m)
        attrs = {attr: getattr(self, name) for attr, name in _OP_ATTRS}      # (read now: an attribute may be assigned after build())
        return dau_conv(inp, w, mu1, mu2, sigma, bias=bias, activation=activation, residual=residual, input_activation=input_activation,
                        number_units_x=self.dau_units[0], number_units_y=self.dau_units[1], sigma_hint=sigma_hint, **attrs)


class DAUConv2d(nn.Module):
    """DAU convolution layer; constructor arguments as in the reference (dau_conv.py:226-258).

    Additions: `in_channels` (build the variables at construction), `algo`, and `check_offsets`: how the op's offset
    preconditions (NaN, |mu| beyond the kernel; dau_conv_op.cpp:250-262) are enforced -- "async" (default): read the
    previous call's on-device result from pinned host memory before each call, no stall, errors surface one call late
    (`dau_conv.check_pending_offsets()` flushes); True: wait for every call and raise at once, as the reference does
    (a call under stream capture cannot wait: there True behaves as "async");
    False: never read the result back.

    Graph capture (`torch.cuda.graph`, `make_graphed_callables`, the cudagraph trees of
    torch.compile): run the layer once before capturing; a captured call reads no sigma on the host, takes its workspace from the
    graph's pool and pins its plan (`dau_conv.release_captured_plans()`); the plan and its prefilter support are frozen in the graph,
    and `dau_conv.check_pending_offsets()` also raises when a replay's sigma needed more taps than the plan holds; a `process_group=`
    layer cannot be captured.

    `dense_split` (None: the library's choice, True: always, False: never): calls whose
    offsets lie within +-2 / +-3 / +-4 run their two gather-sum passes as a densified GEMM on the f16 matrix cores with both
    operands split into two binary16 limbs -- fp32 accuracy (the exact kernels' parity bar), about 1.7x faster at four units per
    channel pair; by default a plan holds the radii that pay for its unit count.  Every image is scaled on its own, so an output
    image (and its input gradient) depends only on that image and the parameters, never on its batch-mates.

    `dense_outliers=True` (opt-in): a call whose
    offsets reach beyond +-3 (up to +-4) in few units -- a trained layer's offsets drift to the +-3.99 clip of kernel 9 -- keeps the
    radius-3 GEMM and gathers those units' outer taps in a sparse pass of its own, instead of moving the whole pass to the 9 x 9
    member; same accuracy, no effect on calls within +-3 or with many such units.

    `dense_line=True` (opt-in, single-dimension layers:
    DAUConv1d, or `dau_unit_single_dim=True`; ValueError elsewhere and together with `dense_split=False` or `dense_bf16=True`): a call whose units all
    lie on the row of their pixel (mu2 == 0) runs its two gather-sum passes as the two-limb GEMM over ONE row of taps -- 1 x 9 for
    offsets within +-4, 1 x 17 within +-8 -- instead of the 9 x 9 kernel or the exact gather; same accuracy; a call with a unit off
    the line runs what it runs without the argument, bit for bit (DAU_FLAG_DENSE_SPLIT_LINE).

    `dense_line_grads=True` (opt-in, the same layers and
    the same ValueErrors): such a call runs its parameter gradients as the line member of the two-limb gather-dot, horizontal radius 4 or 8, in
    place of the exact fp32 gather-dot; fp32 accuracy, independent of `dense_line` (DAU_FLAG_SPLIT_DOT_LINE).

    `dense_bf16=True` (bfloat16 inputs only): calls whose offsets lie within +-4 run
    their forward and input-gradient passes as a densified bf16 matrix-core GEMM (DAU_FLAG_DENSE_BF16: taps and blurred
    activations rounded to bf16, fp32 sums) and, from three units per channel on, their
    parameter gradients as dense cross-correlations on the same cores -- the whole step about 2x faster than the exact
    path at six units, at the bf16 tolerance.

    Activations may be float32, bfloat16 or float16; the output has the input's dtype.  float16 input (torch.autocast("cuda"),
    GradScaler training, `model.half()`) runs the kernels and the fp32 arithmetic of a float32 layer with 16-bit loads and stores
    (DAU_FLAG_IO_F16); the layer casts nothing under autocast.  Parameters of any floating dtype are used as float32 and get
    their gradients in their own dtype.  The bias is added after the op with ordinary type promotion: a float16 (or bfloat16)
    output plus a float32 bias gives a float32 result; after `.half()` the bias is float16 and so is the result.

    `fused_epilogue=True` (default False: the line above): the bias add (when `use_bias`) and the activation, when it is
    `torch.relu`, `torch.nn.functional.relu` or an `nn.ReLU`, run inside the kernels' store -- y = act(sum + bias[f]) in fp32
    before the one rounding -- so the output has the INPUT's dtype (float16 in, float16 out: the next layer keeps its 16-bit loads
    and stores), two whole-tensor passes of the forward step go away, and backward takes the ReLU mask and the bias gradient in one
    pass (the bias gradient stays local, as below).  For float32 the output is bit for bit the unfused one.  Any other activation
    callable is applied after the op; strides > 1 slice the fused result (bias and ReLU commute with the slice); layers whose
    plan has no fused epilogue (shapes on the direct kernels, `dense_bf16=True`) run unfused.

    `channels_last` (None, True, False): what a channels_last input (`x.to(memory_format=torch.channels_last)`; a tensor whose
    strides also fit NCHW -- one channel, or H = W = 1 -- counts as contiguous) runs on.  True: the NHWC plan (DAU_FLAG_IO_NHWC) --
    the same kernels reading and writing [N][H][W][C], no copy of x, which is saved as it is, a channels_last output, and in backward
    a channels_last input gradient from a gradient that is converted only if it is not channels_last already; bit for bit the results
    of the contiguous call.  False: today's path: the input is made contiguous, the output is contiguous.  None (default): the
    NHWC plan for the dtypes where it measured faster than converting (`dau_conv._NHWC_BY_DEFAULT`).  Layers with
    `dense_bf16=True` and shapes that run on the direct kernels have no NHWC plan and convert, whatever the argument.

    `input_activation` (None): an activation applied to the INPUT, in front of the layer.  "relu", `torch.relu`,
    `torch.nn.functional.relu` or an `nn.ReLU` is fused into the layer (DAU_FLAG_INPUT_RELU): in a `Conv2d -> BatchNorm2d -> ReLU ->
    DAUConv2d` stack, drop the ReLU module and give the layer the BatchNorm output -- the kernels clamp x where they load it and mask
    the input gradient by x in its store, so the ReLU's forward and backward passes and its saved output go away; the results are bit
    for bit those of `layer(torch.relu(x))`.  Any other callable is applied in torch before the layer.  Works with channels_last,
    autocast, `.half()` / `.bfloat16()`, `fused_epilogue`, `residual=`, `strides > 1` and `process_group=`; layers whose plan cannot
    take the flag (`dense_bf16=True`, shapes on the direct kernels) run `torch.relu` in front.

    `process_group` (a torch.distributed group, or True for the default one): batch-sharded data parallelism INSIDE the
    layer's backward -- the raw parameter-gradient sums of the local shard are all-reduced (one flat [4,S,G,F] buffer, RCCL
    over xGMI with backend "nccl") while the input gradient is computed, and the elementwise tail runs on the reduced sums;
    weights / mu1 / mu2 / sigma gradients come out identical on every rank, averaged over the ranks (`grad_reduce="mean"`,
    the DistributedDataParallel convention) or summed (`"sum"`).  The bias gradient is ordinary autograd and is not exchanged
    here.  Wrapping such a layer in DistributedDataParallel as well is harmless but redundant (it averages identical values).

    torch.compile: a built layer (`in_channels=` given, or called once) traces into one opaque op, `torch.ops.dau_conv.conv`, with
    the offset clamp, the stride slice and an unfused bias / activation as ordinary traced ops around it; every combination above
    goes through that op, and a trainable sigma does not recompile.  A `process_group=` layer runs outside the graph (one graph
    break; `fullgraph=True` refuses it).  INTEGRATION.md, "torch.compile", has the details.
    """

    # the reference kernels process units in pairs; odd unit counts get one zero-weight ignored unit
    DAU_UNITS_GROUP = 2

    def __init__(self, filters, dau_units, max_kernel_size, strides=1, data_format='channels_first', activation=None,
                 use_bias=True, weight_initializer=None, mu1_initializer=None, mu2_initializer=None,
                 sigma_initializer=None, bias_initializer=None, weight_regularizer=None, mu1_regularizer=None,
                 mu2_regularizer=None, sigma_regularizer=None, bias_regularizer=None, activity_regularizer=None,
                 weight_constraint=None, mu1_constraint=None, mu2_constraint=None, sigma_constraint=None,
                 bias_constraint=None, trainable=True, mu_learning_rate_factor=500, dau_unit_border_bound=0.01,
                 dau_unit_single_dim=False, dau_aggregation_forbid_positive_dim1=False, dau_sigma_trainable=False,
                 dau_mu_interpolation=True, unit_testing=False, name=None, in_channels=None, check_offsets="async",
                 algo=_capi.ALGO_AUTO, dense_bf16=False, process_group=None, grad_reduce="mean", dense_split=None,
                 dense_outliers=False, channels_last=None, fused_epilogue=False, input_activation=None, dense_line=False,
                 dense_line_grads=False, **kwargs):
        super(DAUConv2d, self).__init__()
        _check_line_options(dau_unit_single_dim, dense_split, dense_bf16, dense_line, dense_line_grads)
        self.rank = 2
        self.filters = int(filters)
        du = (dau_units, dau_units) if isinstance(dau_units, int) else tuple(dau_units)
        if len(du) != self.rank:
            raise ValueError("dau_components must be an int or a tuple of %d ints" % self.rank)
        self.dau_units = tuple(int(u) for u in du)
        self.max_kernel_size = max_kernel_size
        self.padding = np.floor(self.max_kernel_size / 2.0)
        self.strides = strides
        if data_format in ("channels_first", "NCHW"):
            self.data_format = "channels_first"
        elif data_format in ("channels_last", "NHWC"):
            self.data_format = "channels_last"
        else:
            raise ValueError("The `data_format` argument must be one of \"channels_first\", \"channels_last\".")
        self.activation = activation
        self.use_bias = bool(use_bias)
        self.trainable = trainable
        self.name = name
        self.weight_initializer = weight_initializer if weight_initializer is not None else random_normal_initializer(stddev=0.1)
        self.bias_initializer = bias_initializer if bias_initializer is not None else zeros_initializer()
        self.mu1_initializer = mu1_initializer
        self.mu2_initializer = mu2_initializer
        self.sigma_initializer = sigma_initializer
        self.regularizers = dict(weights=weight_regularizer, mu1=mu1_regularizer, mu2=mu2_regularizer,
                                 sigma=sigma_regularizer, bias=bias_regularizer)
        self.activity_regularizer = activity_regularizer
        self.constraints = dict(weights=weight_constraint, mu1=mu1_constraint, mu2=mu2_constraint,
                                sigma=sigma_constraint, bias=bias_constraint)
        if self.mu1_initializer is None:
            self.mu1_initializer = DAUGridMean(dau_units=self.dau_units, max_value=np.floor(self.max_kernel_size / 2.0) - 1,
                                               dau_unit_axis=2)
        if self.mu2_initializer is None:
            self.mu2_initializer = DAUGridMean(dau_units=self.dau_units, max_value=np.floor(self.max_kernel_size / 2.0) - 1,
                                               dau_unit_axis=1)
        if self.sigma_initializer is None:
            self.sigma_initializer = constant_initializer(0.5)
        self.mu_learning_rate_factor = mu_learning_rate_factor
        self.unit_testing = unit_testing
        self.dau_unit_border_bound = dau_unit_border_bound
        self.num_dau_units_all = int(np.prod(self.dau_units))
        self.num_dau_units_ignore = 0
        self.dau_mu_interpolation = dau_mu_interpolation
        self.dau_unit_single_dim = dau_unit_single_dim
        self.dau_aggregation_forbid_positive_dim1 = dau_aggregation_forbid_positive_dim1
        self.check_offsets = check_offsets
        self.algo = algo
        self.dense_bf16 = dense_bf16
        self.dense_split = dense_split
        self.dense_outliers = dense_outliers
        self.dense_line = bool(dense_line)
        self.dense_line_grads = bool(dense_line_grads)
        self.channels_last = channels_last
        self.fused_epilogue = bool(fused_epilogue)
        if not (input_activation is None or input_activation == "relu" or callable(input_activation)):
            raise ValueError("input_activation must be None, \"relu\" or a callable")
        self.input_activation = input_activation
        # a ReLU is fused into the op; any other callable runs in torch in front of it
        self._input_relu = (isinstance(input_activation, str) and input_activation == "relu") or \
            input_activation in (torch.relu, nn.functional.relu) or isinstance(input_activation, nn.ReLU)
        self.process_group = process_group
        self.grad_reduce = grad_reduce
        # odd number of units: add one dummy (zero weight, ignored) unit (dau_conv.py:317-329)
        if self.num_dau_units_all % self.DAU_UNITS_GROUP != 0:
            new_num_units = int(np.ceil(self.num_dau_units_all / float(self.DAU_UNITS_GROUP)) * self.DAU_UNITS_GROUP)
            self.num_dau_units_ignore = new_num_units - self.num_dau_units_all
            if self.dau_units[0] < self.dau_units[1]:
                self.dau_units = (self.dau_units[0] + self.num_dau_units_ignore, self.dau_units[1])
            else:
                self.dau_units = (self.dau_units[0], self.dau_units[1] + self.num_dau_units_ignore)
            self.num_dau_units_all = new_num_units
            self.weight_initializer = ZeroNLast(self.weight_initializer, last_num_to_zero=self.num_dau_units_ignore, axis=2)
        self.dau_sigma_trainable = dau_sigma_trainable
        self._manual = {}
        self._sigma_host = None
        self._sigma_tag = None
        self.built = False
        if self.strides > 1:
            warnings.warn('NOTICE: using stride>=2 in DAU convolution uses the same computational resources as with '
                          'stride=1 (current implementation only emulates stride>=2 using tensor slicing).')
        if in_channels is not None:
            self.build((None, int(in_channels), None, None))

    # -- variables --------------------------------------------------------------------------------
    def set_dau_variables_manually(self, w=None, mu1=None, mu2=None, sigma=None):
        """Use caller-provided tensors for w/mu1/mu2/sigma. Call before build() / the first forward."""
        for k, v in (("weights", w), ("mu1", mu1), ("mu2", mu2), ("sigma", sigma)):
            if v is not None:
                self._manual[k] = v

    def _get_input_channel_axis(self):
        if self.data_format == 'channels_first':
            return 1
        raise ValueError('Only `channels_first` supported, i.e., NCHW format.')

    def _get_input_channels(self, input_shape):
        c = input_shape[self._get_input_channel_axis()]
        if c is None:
            raise ValueError('The channel dimension of the inputs should be defined. Found `None`.')
        return int(c)

    def get_dau_variable_shape(self, input_shape):
        return (1, self._get_input_channels(input_shape), self.num_dau_units_all, self.filters)

    def _add(self, name, shape, initializer, trainable=True):
        p = nn.Parameter(_run_init(initializer, shape), requires_grad=bool(trainable and self.trainable))
        self.register_parameter(name, p)
        return p

    def add_dau_weights_var(self, input_shape):
        return self._add('weights', self.get_dau_variable_shape(input_shape), self.weight_initializer)

    def add_dau_mu1_var(self, input_shape):
        return self._add('mu1', self.get_dau_variable_shape(input_shape), self.mu1_initializer)

    def add_dau_mu2_var(self, input_shape):
        return self._add('mu2', self.get_dau_variable_shape(input_shape), self.mu2_initializer)

    def add_dau_sigma_var(self, input_shape, trainable=False):
        # one scalar variable shared by the whole layer (dau_conv.py:417-430)
        return self._add('sigma', (1,), self.sigma_initializer, trainable=trainable)

    def add_bias_var(self):
        return self._add('bias', (self.filters,), self.bias_initializer)

    def build(self, input_shape):
        shape = self.get_dau_variable_shape(input_shape)
        for key, adder in (("weights", self.add_dau_weights_var), ("mu1", self.add_dau_mu1_var),
                           ("mu2", self.add_dau_mu2_var), ("sigma", None)):
            if key in self._manual:
                if tuple(self._manual[key].shape) != tuple(shape):
                    raise ValueError('Shape mismatch for variable `dau_%s`' % key)
            elif adder is not None:
                adder(input_shape)
            else:
                self.add_dau_sigma_var(input_shape, trainable=self.dau_sigma_trainable)
        if self.use_bias:
            self.add_bias_var()
        self._param_shape = shape
        self._dau_convolution_op = _DAUConvolution2d(
            (None, shape[1], None, None), num_output=self.filters, dau_units=self.dau_units,
            max_kernel_size=self.max_kernel_size, padding=self.padding, strides=1,
            num_dau_units_ignore=self.num_dau_units_ignore, mu_learning_rate_factor=self.mu_learning_rate_factor,
            dau_unit_border_bound=self.dau_unit_border_bound, dau_unit_single_dim=self.dau_unit_single_dim,
            dau_aggregation_forbid_positive_dim1=self.dau_aggregation_forbid_positive_dim1,
            dau_mu_interpolation=self.dau_mu_interpolation, unit_testing=self.unit_testing, data_format="NCHW",
            name=self.name, **{option: getattr(self, option) for option in _ENGINE_OPTIONS})
        self.built = True

    def _var(self, key):
        if key in self._manual:
            return self._manual[key]
        return self._parameters.get(key)

    # the reference exposes the variables as op.dau_weights / dau_mu1 / dau_mu2 / dau_sigma
    dau_weights = property(lambda self: self._var("weights"))
    dau_mu1 = property(lambda self: self._var("mu1"))
    dau_mu2 = property(lambda self: self._var("mu2"))
    dau_sigma = property(lambda self: self._var("sigma"))

    def _sigma_tensor_and_hint(self):
        s = self.dau_sigma
        if torch.compiler.is_compiling():
            # the op takes sigma as it is: it tiles a scalar and keeps the host copy itself (_ops._sigma_hint), at run time -- a
            # trainable sigma neither recompiles the graph nor puts an .item() into it
            return s, None
        if s.numel() == 1:
            # tile the scalar to the parameter shape, as the reference graph does (dau_conv.py:429-430)
            # the host copy sizes the prefilter support (2*ceil(5*sigma)+1, base_dau_conv_layer.cpp:146) and keys the plan; it
            # is re-read whenever the tensor has been written since (optimizer step, load_state_dict, constraints,
            # set_dau_variables_manually): the reference re-reads sigma every time it builds its layer (:140-146)
            tag = (s._version, s.data_ptr())
            if self._sigma_host is None or self._sigma_tag != tag:
                if _capi.capturing(s.device):
                    # no host read under stream capture: the most recent copy, whatever the version counter says -- the device
                    # records the support this call's sigma needs (Plan.sigma_status, check_pending_offsets)
                    if self._sigma_host is None:
                        raise _capi.FailedPreconditionError("DAUConv: no host copy of sigma yet; run the layer once before capturing")
                    return s.reshape(1, 1, 1, 1).expand(self._param_shape), self._sigma_host
                self._sigma_host = float(s.detach().reshape(-1)[0].item())
                self._sigma_tag = tag
            return s.reshape(1, 1, 1, 1).expand(self._param_shape), self._sigma_host
        return s, None

    # -- call ---------------------------------------------------------------------------------------
    def forward(self, inputs, residual=None):
        if not self.built:
            self.build(tuple(inputs.shape))
            self.to(inputs.device)
        if inputs.dim() != self.rank + 2:
            raise ValueError('DAU convolution not supported for input with rank %d' % inputs.dim())
        if self.process_group is not None and torch.compiler.is_compiling():
            return _ops.process_group_eager()(DAUConv2d.forward, self, inputs, residual)      # one graph break (see _ops.py)
        sigma_t, hint = self._sigma_tensor_and_hint()
        if self.input_activation is not None and not self._input_relu:
            inputs = self.input_activation(inputs)
        in_act = "relu" if self._input_relu else None

        def op(**epilogue):
            return self._dau_convolution_op(inputs, self.dau_weights, self.dau_mu1, self.dau_mu2, sigma_t, sigma_hint=hint,
                                            input_activation=in_act, **epilogue)
        if self.fused_epilogue:
            # bias and ReLU inside the op's store; both commute with the slicing that emulates strides > 1
            relu = self.activation in (torch.relu, nn.functional.relu) or isinstance(self.activation, nn.ReLU)
            bias = self._parameters["bias"] if self.use_bias else None
            if residual is not None and self.strides > 1:
                # the residual has the SAMPLED shape: the bias stays in the store, the add and the activation follow the slice
                outputs = op(bias=bias)[:, :, ::self.strides, ::self.strides] + residual
                return self.activation(outputs) if self.activation is not None else outputs
            # (a residual joins them in the store: act((sum + bias) + residual); one the op cannot fuse it adds in torch)
            outputs = op(bias=bias, activation="relu" if relu else None, residual=residual)
            if self.strides > 1:
                outputs = outputs[:, :, ::self.strides, ::self.strides]
            if self.activation is not None and not relu:
                return self.activation(outputs)
            return outputs
        outputs = op()
        # strides > 1 are emulated by sampling the stride-1 output (dau_conv.py:497-498)
        if self.strides > 1:
            outputs = outputs[:, :, ::self.strides, ::self.strides]
        if self.use_bias:
            outputs = outputs + self._parameters["bias"].reshape(1, self.filters, 1, 1)
        if residual is not None:
            outputs = outputs + residual
        if self.activation is not None:
            return self.activation(outputs)
        return outputs

    call = forward

    def compute_output_shape(self, input_shape):
        n, _, h, w = input_shape
        return (n, self.filters, int(math.ceil(h / float(self.strides))), int(math.ceil(w / float(self.strides))))

    def regularization_loss(self):
        """Sum of the per-variable regularizers passed to the constructor (TF collected these implicitly)."""
        total = 0.0
        for name, reg in self.regularizers.items():
            p = self._var(name)
            if reg is not None and p is not None:
                total = total + reg(p)
        return total

    @torch.no_grad()
    def apply_constraints(self):
        """Project variables with the constraint callables (TF applied them after each optimizer update)."""
        for name, con in self.constraints.items():
            p = self._var(name)
            if con is not None and p is not None:
                p.copy_(con(p))


class DAUConv1d(DAUConv2d):
    """1-D variant: mu2 fixed at zero, blur only along x (dau_conv.py:557-570)."""

    def __init__(self, filters, dau_units, max_kernel_size, **kwargs):
        def mu_zero_constraint(w):
            return torch.zeros_like(w)
        kwargs.pop("mu2_initializer", None)
        kwargs.pop("mu2_regularizer", None)
        kwargs.pop("mu2_constraint", None)
        kwargs.pop("dau_unit_single_dim", None)
        super(DAUConv1d, self).__init__(filters, dau_units, max_kernel_size, mu2_initializer=zeros_initializer(),
                                        mu2_regularizer=None, mu2_constraint=mu_zero_constraint,
                                        dau_unit_single_dim=True, **kwargs)


# ----------------------------------------------------------------------------------------------
# slim-style functional forms; variables live in a scope-keyed registry (TF: variable_scope + reuse)
# ----------------------------------------------------------------------------------------------
_SCOPES = {}
_SCOPE_COUNTER = [0]


def _scoped_layer(scope, reuse, default_name, factory):
    if scope is None:
        _SCOPE_COUNTER[0] += 1
        scope = default_name if _SCOPE_COUNTER[0] == 1 else "%s_%d" % (default_name, _SCOPE_COUNTER[0] - 1)
    if scope in _SCOPES:
        if reuse is False:
            raise ValueError("Variable scope %s already exists, disallowed. Did you mean to set reuse=True?" % scope)
        return _SCOPES[scope]
    if reuse is True:
        raise ValueError("Variable scope %s does not exist, cannot reuse" % scope)
    layer = factory(scope)
    _SCOPES[scope] = layer
    return layer


def get_scope_layer(scope):
    """The DAUConv2d/1d module that dau_conv2d/dau_conv1d created under `scope` (for optimizers / checkpoints)."""
    return _SCOPES[scope]


def _slim(layer_class, inputs, filters, dau_units, max_kernel_size, data_format, activation_fn, normalizer_fn, normalizer_params,
          fused_epilogue, reuse, outputs_collections, scope, **layer_kwargs):
    """dau_conv2d / dau_conv1d: the layer of this scope -- a layer_class made with layer_kwargs (bias_initializer among them) the
    first time -- applied to inputs, then the normalizer and the activation."""
    if data_format not in [None, 'NCHW']:
        raise ValueError('Invalid data_format: %r' % (data_format,))
    if inputs.dim() != 4:
        raise ValueError('DAU convolution not supported for input with rank', inputs.dim())
    df = 'channels_first' if data_format and data_format.startswith('NC') else 'channels_last'
    # fused_epilogue: the layer itself adds the bias and applies activation_fn (fused where it is a ReLU) -- unless a normalizer
    # stands between them
    fuse_act = bool(fused_epilogue) and normalizer_fn is None and activation_fn is not None
    layer = _scoped_layer(scope, reuse, 'DAUConv', lambda name: layer_class(
        filters, dau_units, max_kernel_size, data_format=df, activation=activation_fn if fuse_act else None,
        fused_epilogue=fused_epilogue, use_bias=bool(not normalizer_fn and layer_kwargs["bias_initializer"]), unit_testing=False,
        name=name, **layer_kwargs))
    outputs = layer(inputs)
    if normalizer_fn is not None:
        outputs = normalizer_fn(outputs, **(normalizer_params or {}))
    if activation_fn is not None and not fuse_act:
        outputs = activation_fn(outputs)
    if outputs_collections is not None:
        outputs_collections.append(outputs)
    return outputs


def dau_conv2d(inputs, filters, dau_units, max_kernel_size, stride=1, mu_learning_rate_factor=500, data_format=None,
               activation_fn=torch.relu, normalizer_fn=None, normalizer_params=None, weights_initializer=None,
               weights_regularizer=None, weights_constraint=None, mu1_initializer=None, mu1_regularizer=None,
               mu1_constraint=None, mu2_initializer=None, mu2_regularizer=None, mu2_constraint=None,
               sigma_initializer=None, sigma_regularizer=None, sigma_constraint=None, biases_initializer=zeros_initializer(),
               biases_regularizer=None, biases_constraint=None, dau_unit_border_bound=0.01, dau_sigma_trainable=False,
               dau_mu_interpolation=True, reuse=None, variables_collections=None, outputs_collections=None,
               trainable=True, scope=None, dense_outliers=False, fused_epilogue=False, input_activation_fn=None):
    """slim-style functional form of DAUConv2d.  Its variables live in a Python-side scope registry (_SCOPES), which Dynamo does not
    trace: dau_conv2d / dau_conv1d stay eager -- under torch.compile, build the model from the DAUConv2d / DAUConv1d modules."""
    return _slim(
        DAUConv2d, inputs, filters, dau_units, max_kernel_size, data_format, activation_fn, normalizer_fn, normalizer_params,
        fused_epilogue, reuse, outputs_collections, scope, strides=stride, mu_learning_rate_factor=mu_learning_rate_factor,
        weight_initializer=weights_initializer, mu1_initializer=mu1_initializer, mu2_initializer=mu2_initializer,
        sigma_initializer=sigma_initializer, bias_initializer=biases_initializer, weight_regularizer=weights_regularizer,
        mu1_regularizer=mu1_regularizer, mu2_regularizer=mu2_regularizer, sigma_regularizer=sigma_regularizer,
        bias_regularizer=biases_regularizer, weight_constraint=weights_constraint, mu1_constraint=mu1_constraint,
        mu2_constraint=mu2_constraint, sigma_constraint=sigma_constraint, bias_constraint=biases_constraint,
        dau_unit_border_bound=dau_unit_border_bound, dau_sigma_trainable=dau_sigma_trainable,
        dau_mu_interpolation=dau_mu_interpolation, trainable=trainable, dense_outliers=dense_outliers,
        input_activation=input_activation_fn)


def dau_conv1d(inputs, filters, dau_units, max_kernel_size, stride=1, mu_learning_rate_factor=500, data_format=None,
               activation_fn=torch.relu, normalizer_fn=None, normalizer_params=None, weights_initializer=None,
               weights_regularizer=None, weights_constraint=None, mu1_initializer=None, mu1_regularizer=None,
               mu1_constraint=None, sigma_initializer=None, sigma_regularizer=None, sigma_constraint=None,
               biases_initializer=zeros_initializer(), biases_regularizer=None, dau_unit_border_bound=0.01,
               dau_sigma_trainable=False, dau_aggregation_forbid_positive_dim1=False, dau_mu_interpolation=True,
               reuse=None, variables_collections=None, outputs_collections=None, trainable=True, scope=None,
               dense_outliers=False, fused_epilogue=False, input_activation_fn=None, dense_line=False, dense_line_grads=False):
    """slim-style functional form of DAUConv1d; like dau_conv2d it keeps its variables in the Python-side scope registry and stays
    eager under torch.compile."""
    return _slim(
        DAUConv1d, inputs, filters, dau_units, max_kernel_size, data_format, activation_fn, normalizer_fn, normalizer_params,
        fused_epilogue, reuse, outputs_collections, scope, strides=stride, mu_learning_rate_factor=mu_learning_rate_factor,
        weight_initializer=weights_initializer, mu1_initializer=mu1_initializer, sigma_initializer=sigma_initializer,
        bias_initializer=biases_initializer, weight_regularizer=weights_regularizer, mu1_regularizer=mu1_regularizer,
        sigma_regularizer=sigma_regularizer, bias_regularizer=biases_regularizer, weight_constraint=weights_constraint,
        mu1_constraint=mu1_constraint, sigma_constraint=sigma_constraint, dau_unit_border_bound=dau_unit_border_bound,
        dau_sigma_trainable=dau_sigma_trainable, dau_aggregation_forbid_positive_dim1=dau_aggregation_forbid_positive_dim1,
        dau_mu_interpolation=dau_mu_interpolation, trainable=trainable, dense_outliers=dense_outliers,
        input_activation=input_activation_fn, dense_line=dense_line, dense_line_grads=dense_line_grads)


# the opaque ops of the torch.compile path; imported last: _ops.py uses this module's helpers
from . import _ops  # noqa: E402
