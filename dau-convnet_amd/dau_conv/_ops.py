"""The DAU operator as two opaque PyTorch ops, `dau_conv::conv` and `dau_conv::conv_backward` (torch.library.custom_op), so that a
layer can sit inside `torch.compile`: Dynamo sees one op with a shape function, and everything that depends on the plan -- the plan
cache, the library's refusals and the fallbacks they select, the offset status, the host copy of sigma -- happens at run time inside
the op's implementation, where the tensors are real.  The forward and the backward over a plan are dau_conv.py's _forward / _backward,
the core the eager layer's _DAUConvFunction runs as well (eager calls it directly, never through these ops: no dispatcher cost, and the
two promise rules below are the ops' alone).  What the implementations here add around that core: sigma tiled and its host copy kept
(_tiled, _sigma_hint); what a plan does not fuse -- `+ bias`, `+ residual`, ReLU, the ReLU in front -- applied in torch inside the op,
forward and backward, where eager leaves it to torch's autograd outside its function; the result brought to the shape function's
promise (_promised); grad cast to x's dtype; 0-element tensors for the gradients not asked for.

    conv(x, w, mu1, mu2, sigma, bias?, residual?, relu, input_relu, ...settings...) -> y
        y = act((DAU(relu?(x)) + bias[f]) + residual): what dau_conv() computes for these arguments.  w, mu1, mu2 [1,S,G,F]; sigma
        [1,S,G,F], or one element that the op tiles; the parameters and the bias of any floating dtype (used as float32).
        residual, when given, has y's shape and x's dtype (dau_conv() adds any other residual in torch, outside the op).
    conv_backward(grad, x, w, mu1, mu2, sigma, y?, relu, input_relu, need_mask, need_dbias, ...settings...)
        -> (dx, dw, dmu1, dmu2, dsigma, dbias): need_mask holds the _capi.NEED_* bits; a gradient that is not asked for comes back as
        a 0-element tensor.  x is the raw input (of an input_relu call too), y the forward's output, needed with relu only.
    settings: number_units_ignore, kernel_size, unit_testing, mu_learning_rate_factor, single_dim_kernel, forbid_positive_dim1,
        use_interpolation, algo (the _capi.ALGO_* value, plus 16 with dense_line_grads=True: the line members of the two-limb gather-dot
        -- the schema has no argument of its own for it either), dense_bf16, dense_split (-1: the library's choice, 0: never, 1: always; 2: the library's choice plus
        the line members of dense_line=True, 3: always plus the line members -- the schema has no argument of its own for it), dense_outliers,
        channels_last (-1: by dtype, 0, 1) and check_offsets ("async", "on", "off") -- what _settings() normalises, as schema types.

What the shape functions promise, from dtypes, strides and arguments alone:
    y       [N, F, H, W] in x's dtype; channels_last exactly when _wants_nhwc(x, settings) holds, contiguous otherwise
    dx      like x, in the format of y's rule
    dw, dmu1, dmu2, dsigma   [1, S, G, F] float32;  dbias  [F] float32
Two of today's eager rules depend on the plan, and the implementations bring their results to the promise instead:
  * a plan without the fused epilogue (shapes on the direct kernels, dense_bf16) adds the bias in torch, where eager lets torch promote
    -- a bfloat16 output plus a float32 bias is float32 in eager.  Here the sum is rounded to x's dtype, the fused epilogue's rule.
    Where the bias has x's dtype (after .half() / .bfloat16()) or x is float32 the two agree bit for bit;
  * a channels_last input whose NHWC plan the library refuses (the direct-kernel shapes) gives a contiguous output in eager.  Here
    the output and the input gradient are converted to channels_last."""
import collections
import weakref

import torch

from . import _capi
from . import dau_conv as _impl

_TRI = {None: -1, False: 0, True: 1}
_UNTRI = {-1: None, 0: False, 1: True}
# the op's integer dense_split carries dense_line too: (dense_split, dense_line) <-> -1, 0, 1 as above, 2, 3 with the line members
_SPLIT = {(None, False): -1, (False, False): 0, (True, False): 1, (None, True): 2, (True, True): 3}
_UNSPLIT = {v: k for k, v in _SPLIT.items()}
_LINE_GRADS = 16                     # the op's integer algo carries dense_line_grads: algo + 16
_CHECK = {"async": "async", True: "on", False: "off"}
_UNCHECK = {"async": "async", "on": True, "off": False}


def _untri(channels_last):
    if channels_last not in _UNTRI:
        raise _capi.InvalidArgumentError("channels_last must be -1 (by dtype), 0 or 1")
    return _UNTRI[channels_last]


# One trailing argument of the ops.  type: its schema type; encode: the argument from a _settings() dict; decode: the _settings()
# keywords from the argument
_Setting = collections.namedtuple("_Setting", "name type encode decode")


def _as_is(name, type):
    return _Setting(name, type, lambda st: st[name], lambda v: {name: v})


# The ops' settings, in schema order: all that encode_settings, _run_settings, the schemas' tails and _N_ARGS know of them
_SETTINGS = (
    _as_is("number_units_ignore", "SymInt"), _as_is("kernel_size", "SymInt"), _as_is("unit_testing", "bool"),
    _as_is("mu_learning_rate_factor", "float"), _as_is("single_dim_kernel", "bool"), _as_is("forbid_positive_dim1", "bool"),
    _as_is("use_interpolation", "bool"),
    # (the two packed pairs: the schema has no argument of its own for dense_line_grads, nor for dense_line below)
    _Setting("algo", "SymInt", lambda st: st["algo"] + (_LINE_GRADS if st["dense_line_grads"] else 0),
             lambda v: dict(algo=v & ~_LINE_GRADS, dense_line_grads=bool(v & _LINE_GRADS))),
    _as_is("dense_bf16", "bool"),
    _Setting("dense_split", "SymInt", lambda st: _SPLIT[(st["dense_split"], st["dense_line"])],
             lambda v: dict(zip(("dense_split", "dense_line"), _UNSPLIT[v]))),
    _as_is("dense_outliers", "bool"),
    _Setting("channels_last", "SymInt", lambda st: _TRI[st["channels_last"]], lambda v: dict(channels_last=_untri(v))),
    _Setting("check_offsets", "str", lambda st: _CHECK[st["check_offsets"]], lambda v: dict(check_offsets=_UNCHECK[v])))
_NAMES = tuple(s.name for s in _SETTINGS)
_SCHEMA_TAIL = ", ".join("%s %s" % (s.type, s.name) for s in _SETTINGS)


def encode_settings(st):
    """The op's trailing arguments from a _settings() dict, in schema order."""
    return tuple(s.encode(st) for s in _SETTINGS)


def _layout_settings(dense_bf16, channels_last):
    """All of the settings that _wants_nhwc reads."""
    return dict(dense_bf16=bool(dense_bf16), channels_last=_untri(channels_last))


def _tail_layout(tail):
    """_layout_settings of an op's trailing arguments: all a shape function reads of them."""
    return _layout_settings(tail[_NAMES.index("dense_bf16")], tail[_NAMES.index("channels_last")])


# ----------------------------------------------------------------------------------------------
# the host copy of sigma that sizes the prefilter support and keys the plan
# ----------------------------------------------------------------------------------------------
# Per sigma tensor, as DAUConv2d._sigma_tensor_and_hint keeps it for the eager layer: re-read when the tensor has been written since
# (its version counter) or is another tensor (the object itself, held weakly, and its address), so a fixed sigma costs one read in
# all and a trainable one a read per optimizer step -- outside the graph either way.  Bounded, least recently used.
_SIGMA_HOST = collections.OrderedDict()
_SIGMA_HOST_MAX = 256


def _read_sigma(sigma):
    return float(sigma.detach().reshape(-1)[0].item())


def _sigma_hint(sigma, every_call=False, like=None):
    """every_call: read whatever the copy says, as a full sigma tensor is read (eager's _settings() without a sigma_hint).
    Under stream capture nothing is read: the most recent copy kept for the tensor at this address, whatever its version counter
    says -- the device records the support the call's sigma needs (Plan.sigma_status, check_pending_offsets).
    like: what the op knows of its layer (device, parameter shape, kernel settings).  A graph runner that copies its inputs into
    buffers of its own (the cudagraph trees behind torch.compile(backend="cudagraphs") do so with parameters) records the op with a
    sigma at an address no call has read: it then takes the most recent copy an ordinary call `like` it kept -- the warm-up run of
    the same graph, just before the recording.  LIMIT: two layers alike in all of that whose sigmas need different supports cannot
    be told apart there (the op sees copies of every parameter): the one that ran earlier records with the later one's support.
    Too few taps are reported by the device's record (check_pending_offsets raises); too many are a correct but wider truncation
    than the eager layer's.  Runners that hand the op its own parameters (torch.cuda.graph, make_graphed_callables, Inductor's
    trees, which treat parameters as static) never take this path."""
    every_call = every_call or sigma.numel() != 1     # a full sigma tensor: the read _settings() performs on every eager call
    key = (sigma.data_ptr(), sigma.device.index)
    hit = _SIGMA_HOST.get(key)
    if not every_call and hit is not None and hit[0]() is sigma and hit[1] == sigma._version:
        _SIGMA_HOST.move_to_end(key)
        if like is not None:                 # (the most recent ordinary call like this one, also when it read nothing)
            _SIGMA_HOST[like] = (_NO_TENSOR, -1, hit[2])
            _SIGMA_HOST.move_to_end(like)
        return hit[2]
    if _capi.capturing(sigma.device):
        if hit is None and like is not None:
            hit = _SIGMA_HOST.get(like)
        if hit is None:
            raise _capi.FailedPreconditionError("DAUConv: no host copy of sigma yet; run the layer once before capturing")
        return hit[2]
    value = _read_sigma(sigma)
    _SIGMA_HOST[key] = (weakref.ref(sigma), sigma._version, value)
    _SIGMA_HOST.move_to_end(key)
    if like is not None:
        _SIGMA_HOST[like] = (_NO_TENSOR, -1, value)
        _SIGMA_HOST.move_to_end(like)
    while len(_SIGMA_HOST) > _SIGMA_HOST_MAX:
        _SIGMA_HOST.popitem(last=False)
    return value


def _NO_TENSOR():
    return None


def _run_settings(w, sigma, input_relu, *tail):
    """The _settings() dict of a real call, from the op's trailing arguments."""
    arg = dict(zip(_NAMES, tail, strict=True))
    if arg["dense_split"] not in _UNSPLIT or arg["check_offsets"] not in _UNCHECK:
        raise _capi.InvalidArgumentError("dense_split must be -1, 0, 1, 2 or 3 and check_offsets \"async\", \"on\" or \"off\"")
    attrs = dict(num_output=w.shape[-1], sigma_hint=_sigma_hint(sigma, like=("like", sigma.device.index, tuple(w.shape)) + tuple(
        arg[n] for n in ("kernel_size", "number_units_ignore", "single_dim_kernel", "forbid_positive_dim1", "use_interpolation"))))
    for s in _SETTINGS:
        attrs.update(s.decode(arg[s.name]))
    st = _impl._settings(sigma, **attrs)
    st["input_relu"] = bool(input_relu)
    return st


def _tiled(sigma, w):
    """sigma as the kernels take it: contiguous float32 [1,S,G,F]; one element is tiled."""
    sigma = _impl._f32(sigma)
    if sigma.numel() == 1 and w.numel() != 1:
        sigma = sigma.reshape(1, 1, 1, 1).expand(w.shape)
    return _impl._c(sigma)


def _promised(t, nhwc, dtype):
    """t in the dtype and with the strides the shape function gave: those of torch.empty in that memory format."""
    if t.dtype != dtype:
        t = t.to(dtype)
    n, c, h, w = t.shape
    if tuple(t.stride()) == ((h * w * c, 1, w * c, c) if nhwc else (c * h * w, h * w, w, 1)):
        return t
    return _empty_act(t, tuple(t.shape), nhwc).copy_(t)


def _empty_act(like, shape, nhwc):
    return torch.empty(shape, dtype=like.dtype, device=like.device,
                       memory_format=torch.channels_last if nhwc else torch.contiguous_format)


def _check_shapes(x, w, residual=None):
    if x.dim() != 4 or w.dim() != 4:
        raise _capi.InvalidArgumentError("dau_conv: the input must be [N,S,H,W] and the parameters [1,S,G,F]")
    if residual is not None and not (residual.dtype == x.dtype and residual.dim() == 4):
        raise _capi.InvalidArgumentError("dau_conv::conv: the residual must have the input's dtype and the output's shape")


# ----------------------------------------------------------------------------------------------
# dau_conv::conv
# ----------------------------------------------------------------------------------------------
@torch.library.custom_op("dau_conv::conv", mutates_args=(), schema="(Tensor x, Tensor w, Tensor mu1, Tensor mu2, Tensor sigma, "
                         "Tensor? bias, Tensor? residual, bool relu, bool input_relu, " + _SCHEMA_TAIL + ") -> Tensor")
def conv(x, w, mu1, mu2, sigma, bias, residual, relu, input_relu, *tail):
    _check_shapes(x, w, residual)
    st = _run_settings(w, sigma, input_relu, *tail)
    nhwc = _impl._wants_nhwc(x, st)
    w, mu1, mu2 = (_impl._c(_impl._f32(t)) for t in (w, mu1, mu2))
    sigma = _tiled(sigma, w)
    _impl._check_bias(bias, w)
    if residual is not None and not _impl._residual_fusable(residual, x, w):
        raise _capi.InvalidArgumentError("dau_conv::conv: the residual must have the input's dtype and the output's shape")
    plan = _impl._get_plan(x, w, st, nhwc)
    if input_relu and not plan.input_relu:
        x = torch.relu(x)                    # the plan cannot take the flag (direct kernels, dense_bf16): the ReLU in front
    if not (bias is not None or relu or residual is not None) or _impl._epilogue_ok(plan):
        y = _impl._forward(plan, st, x, w, mu1, mu2, sigma, None if bias is None else _impl._c(_impl._f32(bias)), relu, residual)[0]
    else:
        # no fused epilogue: the op, then `+ bias`, `+ residual` and relu in torch, in dau_conv()'s order
        y = _impl._forward(plan, st, x, w, mu1, mu2, sigma)[0]
        if bias is not None:
            y = y + bias.reshape(1, -1, 1, 1)
        if residual is not None:
            y = y + residual
        if relu:
            y = torch.relu(y)
    return _promised(y, nhwc, x.dtype)


@conv.register_fake
def _conv_fake(x, w, mu1, mu2, sigma, bias, residual, relu, input_relu, *tail):
    _check_shapes(x, w, residual)
    nhwc = _impl._wants_nhwc(x, _tail_layout(tail))
    return _empty_act(x, (x.shape[0], w.shape[-1], x.shape[2], x.shape[3]), nhwc)


# ----------------------------------------------------------------------------------------------
# dau_conv::conv_backward
# ----------------------------------------------------------------------------------------------
@torch.library.custom_op("dau_conv::conv_backward", mutates_args=(), schema="(Tensor grad, Tensor x, Tensor w, Tensor mu1, Tensor mu2, "
                         "Tensor sigma, Tensor? y, bool relu, bool input_relu, SymInt need_mask, bool need_dbias, " + _SCHEMA_TAIL +
                         ") -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
def conv_backward(grad, x, w, mu1, mu2, sigma, y, relu, input_relu, need_mask, need_dbias, *tail):
    _check_shapes(x, w)
    if relu and y is None:
        raise _capi.InvalidArgumentError("dau_conv::conv_backward: relu needs the forward's output")
    st = _run_settings(w, sigma, input_relu, *tail)
    nhwc = _impl._wants_nhwc(x, st)
    w, mu1, mu2 = (_impl._c(_impl._f32(t)) for t in (w, mu1, mu2))
    sigma = _tiled(sigma, w)
    plan = _impl._get_plan(x, w, st, nhwc)
    relu_in_front = input_relu and not plan.input_relu
    if relu_in_front:
        x = torch.relu(x)
    none = lambda like, dtype=torch.float32: torch.empty((0,), dtype=dtype, device=like.device)
    need = int(need_mask) & _capi.NEED_ALL
    if need == 0 and not need_dbias:
        return (none(x, x.dtype),) + (none(x),) * 5
    grad = _impl._act(grad if grad.dtype == x.dtype else grad.to(x.dtype), plan)
    if (need_dbias or relu) and not _impl._epilogue_ok(plan):
        # no fused epilogue: its backward in torch -- the select threshold_backward makes, the sum `+ bias`'s autograd makes
        if relu:
            grad = torch.where(_impl._act(y, plan) <= 0, torch.zeros((), dtype=grad.dtype, device=grad.device), grad)
        dbias = grad.sum_to_size(1, grad.shape[1], 1, 1).reshape(-1).float() if need_dbias else None
        out = _impl._backward(plan, st, _impl._act(x, plan), grad, w, mu1, mu2, sigma, need)[2]
    else:
        _, dbias, out = _impl._backward(plan, st, _impl._act(x, plan), grad, w, mu1, mu2, sigma, need, y, relu, need_dbias)
    dx = out[0]
    if dx is not None:
        if relu_in_front:
            dx = torch.where(x <= 0, torch.zeros((), dtype=dx.dtype, device=dx.device), dx)
        dx = _promised(dx, nhwc, x.dtype)
    return (none(x, x.dtype) if dx is None else dx,) + tuple(none(x) if t is None else t for t in out[1:]) + \
        (none(x) if dbias is None else dbias,)


@conv_backward.register_fake
def _conv_backward_fake(grad, x, w, mu1, mu2, sigma, y, relu, input_relu, need_mask, need_dbias, *tail):
    _check_shapes(x, w)
    nhwc = _impl._wants_nhwc(x, _tail_layout(tail))
    f32 = lambda shape: torch.empty(shape, dtype=torch.float32, device=x.device)
    need = int(need_mask) & _capi.NEED_ALL
    pshape = (1, w.shape[1], w.shape[2], w.shape[3])
    dx = _empty_act(x, tuple(x.shape), nhwc) if need & _capi.NEED_DX else torch.empty((0,), dtype=x.dtype, device=x.device)
    params = tuple(f32(pshape) if need & bit else f32((0,))
                   for bit in (_capi.NEED_DW, _capi.NEED_DMU1, _capi.NEED_DMU2, _capi.NEED_DSIGMA))
    return (dx,) + params + (f32((w.shape[-1],)) if need_dbias else f32((0,)),)


# ----------------------------------------------------------------------------------------------
# autograd of dau_conv::conv
# ----------------------------------------------------------------------------------------------
_N_ARGS = 9 + len(_SETTINGS)         # x, w, mu1, mu2, sigma, bias, residual, relu, input_relu and the settings


def _setup_context(ctx, inputs, output):
    x, w, mu1, mu2, sigma, bias, residual, relu, input_relu = inputs[:9]
    # the raw input (an input_relu call's ReLU output is never materialised, nor saved) and y only for the ReLU mask
    ctx.save_for_backward(*((x, w, mu1, mu2, sigma) + ((output,) if relu else ())))
    ctx.relu, ctx.input_relu, ctx.settings = bool(relu), bool(input_relu), tuple(inputs[9:])
    ctx.need = _impl._need_mask(ctx.needs_input_grad)
    ctx.need_dbias = bias is not None and bool(ctx.needs_input_grad[5])
    ctx.need_dres = residual is not None and bool(ctx.needs_input_grad[6])
    ctx.param_dtypes = tuple(t.dtype for t in (w, mu1, mu2, sigma))
    ctx.bias_dtype = None if bias is None else bias.dtype
    ctx.sigma_shape = tuple(sigma.shape)


def _backward(ctx, grad):
    x, w, mu1, mu2, sigma = ctx.saved_tensors[:5]
    y = ctx.saved_tensors[5] if ctx.relu else None
    grads = [None] * _N_ARGS
    if ctx.need == 0 and not ctx.need_dbias and not ctx.need_dres:
        return tuple(grads)
    if ctx.need_dres:
        # the residual joins the sum before the activation: its gradient IS the gradient of the sum -- grad itself, or with a ReLU
        # the masked grad (the select the op's epilogue pass computes: no arithmetic, the same bits)
        grads[6] = grad if not ctx.relu else torch.where(y <= 0, torch.zeros((), dtype=grad.dtype, device=grad.device), grad)
    if ctx.need or ctx.need_dbias:
        out = torch.ops.dau_conv.conv_backward(grad, x, w, mu1, mu2, sigma, y, ctx.relu, ctx.input_relu, ctx.need, ctx.need_dbias,
                                               *ctx.settings)
        if ctx.need & _capi.NEED_DX:
            grads[0] = out[0]
        for i, bit in enumerate((_capi.NEED_DW, _capi.NEED_DMU1, _capi.NEED_DMU2, _capi.NEED_DSIGMA)):
            if ctx.need & bit:
                g = out[1 + i]
                if i == 3 and tuple(g.shape) != ctx.sigma_shape:
                    g = g.sum_to_size(1, 1, 1, 1).reshape(ctx.sigma_shape)       # a tiled scalar: the sum over its copies
                grads[1 + i] = g if g.dtype == ctx.param_dtypes[i] else g.to(ctx.param_dtypes[i])
        if ctx.need_dbias:
            grads[5] = out[5] if out[5].dtype == ctx.bias_dtype else out[5].to(ctx.bias_dtype)
    return tuple(grads)


conv.register_autograd(_backward, setup_context=_setup_context)


# ----------------------------------------------------------------------------------------------
# process_group= layers under torch.compile
# ----------------------------------------------------------------------------------------------
_PROCESS_GROUP_EAGER = []


def process_group_eager():
    """-> call(fn, *args, **kwargs) that runs fn (today's dau_conv(), or a layer's forward) outside the graph: the overlapped
    all-reduce of a process_group= layer's backward is not an op.  One graph break per call; fullgraph=True refuses it, naming
    process_group.  Built on first use (a layer with process_group=
    builds it at construction): torch._dynamo is not imported with the package."""
    if not _PROCESS_GROUP_EAGER:
        import torch._dynamo

        def dau_conv_process_group_eager(fn, *args, **kwargs):
            return fn(*args, **kwargs)

        _PROCESS_GROUP_EAGER.append(torch._dynamo.disable(
            dau_conv_process_group_eager, reason="DAUConv with process_group= runs its overlapped all-reduce backward in eager"))
    return _PROCESS_GROUP_EAGER[0]
