"""ctypes binding of the C ABI in include/dau_conv.h (libdau_conv_hip.so).

This is the only route from Python into the operator: there is no CPU or eager-PyTorch
fallback.  If the HIP library is missing the import fails loudly.
PyTorch is used for device memory and the current HIP stream only.
"""
import collections
import ctypes
import os
import sys
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DAU_CONV_LIB selects another build of the same ABI (A/B timing of kernel variants on one device)
_LIB_PATH = os.environ.get("DAU_CONV_LIB") or os.path.join(_HERE, "libdau_conv_hip.so")

DAU_OK, DAU_INVALID_ARGUMENT, DAU_FAILED_PRECONDITION, DAU_INTERNAL = 0, 1, 2, 3

FLAG_USE_INTERPOLATION = 1 << 0
FLAG_UNIT_TESTING = 1 << 1
FLAG_SINGLE_DIM_KERNEL = 1 << 2
FLAG_FORBID_POSITIVE_DIM1 = 1 << 3
FLAG_IO_BF16 = 1 << 4   # x, y, dy, dx are torch.bfloat16; parameters and their gradients stay float32
FLAG_STATIC_BUCKET = 1 << 5   # always the kernels of the bucket max_kernel_size allows (no per-call selection)
FLAG_DENSE_BF16 = 1 << 6      # with FLAG_IO_BF16: gather-sum passes of calls with |mu| <= 4 as a densified bf16 MFMA GEMM
FLAG_DENSE_WGRAD_NEVER = 1 << 7    # with FLAG_DENSE_BF16: parameter gradients always through the exact fp32 gather-dot
FLAG_DENSE_WGRAD_ALWAYS = 1 << 8   # with FLAG_DENSE_BF16: dense parameter gradients from one unit per channel on (default: three)
FLAG_DENSE_SPLIT_F16 = 1 << 9      # gather-sum passes of calls with |mu| <= 2 / 3 / 4 as a densified two-limb f16 MFMA GEMM at fp32 accuracy, whatever G
FLAG_NO_DENSE_SPLIT = 1 << 10      # never (default: the radii that pay for the plan's unit count)
FLAG_DENSE_SPLIT_LINE = 1 << 15       # opt-in, with FLAG_SINGLE_DIM_KERNEL: calls whose units lie on a line run the 1 x 9 / 1 x 17 two-limb GEMM
FLAG_SPLIT_DOT_LINE = 1 << 16         # opt-in, with FLAG_SINGLE_DIM_KERNEL: parameter gradients of calls whose units lie on a line run the line member of the two-limb gather-dot
FLAG_DENSE_SPLIT_OUTLIERS = 1 << 12   # opt-in: calls within +-4 with few units beyond +-3 run the radius-3 two-limb GEMM plus a sparse ring pass
FLAG_IO_F16 = 1 << 11   # x, y, dy, dx are torch.float16; the fp32 plan's kernels and arithmetic, parameters and their gradients float32
FLAG_IO_NHWC = 1 << 13  # x, y, dy, dx are channels_last: [N][H][W][C] in memory; the NCHW plan of the same desc in everything but addresses
FLAG_INPUT_RELU = 1 << 14   # a ReLU in front of the layer, fused: x is clamped at zero where the kernels load it, dx is masked by x in its store

ALGO_AUTO, ALGO_DIRECT, ALGO_TILED = 0, 1, 2
PASS_FORWARD, PASS_BACKWARD, PASS_EPILOGUE_BACKWARD = 1, 2, 3
EPILOGUE_BIAS, EPILOGUE_RELU = 1, 2   # fused into the forward store: y = act(sum + bias[f]) in fp32 before the one rounding
NEED_DX, NEED_DW, NEED_DMU1, NEED_DMU2, NEED_DSIGMA, NEED_ALL = 1, 2, 4, 8, 16, 31


class DAUConvError(RuntimeError):
    """Base class; .code holds the DAU_* status."""
    code = DAU_INTERNAL


class InvalidArgumentError(DAUConvError, ValueError):      # TF: errors.InvalidArgumentError
    code = DAU_INVALID_ARGUMENT


class FailedPreconditionError(DAUConvError):                # TF: errors.FailedPreconditionError
    code = DAU_FAILED_PRECONDITION


class InternalError(DAUConvError):                          # TF: errors.InternalError
    code = DAU_INTERNAL


class _Desc(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("batch", ctypes.c_int32), ("in_channels", ctypes.c_int32),
        ("out_channels", ctypes.c_int32), ("units_per_channel", ctypes.c_int32), ("height", ctypes.c_int32),
        ("width", ctypes.c_int32), ("max_kernel_size", ctypes.c_int32), ("number_units_ignore", ctypes.c_int32),
        ("flags", ctypes.c_int32), ("algo", ctypes.c_int32), ("sigma_hint", ctypes.c_float),
        ("mu_learning_rate_factor", ctypes.c_float),
    ]


class _Info(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("offset_bucket", "blur_support", "algo_forward", "algo_backward", "drop_last_col", "drop_last_row",
                 "gather_patch", "gather_stack", "dot_windows", "gather_windows", "bucket_sets", "gather_dense_bf16", "batch_slab_gather", "batch_slab_dot", "dot_region", "gather_fblock", "gather_variant", "dense_bf16_radius3", "gather_dense_split")]


def _load():
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            "dau_conv: %s not found. Build it with `make -C dau-convnet_amd/csrc` (hipcc, gfx950) or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback." % _LIB_PATH)
    lib = ctypes.CDLL(_LIB_PATH)
    vp, fp, ip = ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p
    lib.dau_conv_abi_version.restype = ctypes.c_int
    lib.dau_conv_last_error.restype = ctypes.c_char_p
    lib.dau_conv_build_id.restype = ctypes.c_char_p
    lib.dau_conv_plan_create.argtypes = [ctypes.POINTER(_Desc), ctypes.POINTER(vp)]
    lib.dau_conv_plan_destroy.argtypes = [vp]
    lib.dau_conv_plan_get_info.argtypes = [vp, ctypes.POINTER(_Info)]
    lib.dau_conv_workspace_bytes.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    lib.dau_conv_forward.argtypes = [vp, vp, fp, fp, fp, fp, fp, fp, vp, ctypes.c_size_t]
    lib.dau_conv_backward.argtypes = [vp, vp] + [fp] * 11 + [vp, ctypes.c_size_t, ctypes.c_int]
    lib.dau_conv_backward_param_sums.argtypes = [vp, vp] + [fp] * 6 + [vp, ctypes.c_size_t]
    lib.dau_conv_finalize_param_grads.argtypes = [vp, vp] + [fp] * 6 + [ctypes.c_int]
    lib.dau_conv_check_status.argtypes = [vp, vp, vp, ctypes.POINTER(ctypes.c_float)]
    if hasattr(lib, "dau_conv_gather_outlier_status"):   # (an earlier build of the same ABI, loaded through DAU_CONV_LIB for an A/B run, lacks the query)
        lib.dau_conv_gather_outlier_status.argtypes = [vp, vp, vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    if hasattr(lib, "dau_conv_gather_line_status"):      # (likewise: the line members' query)
        lib.dau_conv_gather_line_status.argtypes = [vp, vp, vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    if hasattr(lib, "dau_conv_dot_line_status"):         # (likewise: the gather-dot's line members' query)
        lib.dau_conv_dot_line_status.argtypes = [vp, vp, vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    if hasattr(lib, "dau_conv_split_dot_geometry"):      # (likewise: the split gather-dot's strip geometry)
        lib.dau_conv_split_dot_geometry.argtypes = [vp] + [ctypes.POINTER(ctypes.c_int32)] * 3
    if hasattr(lib, "dau_conv_forward_epilogue"):        # (likewise: the fused epilogue and its backward pass)
        lib.dau_conv_epilogue_supported.argtypes = [vp, ctypes.c_int]
        lib.dau_conv_forward_epilogue.argtypes = [vp, vp, fp, fp, fp, fp, fp, fp, ctypes.c_int, fp, vp, ctypes.c_size_t]
        lib.dau_conv_epilogue_backward.argtypes = [vp, vp, fp, fp, ctypes.c_int, fp, fp, vp, ctypes.c_size_t]
    if hasattr(lib, "dau_conv_forward_residual"):        # (likewise: the residual add of that epilogue)
        lib.dau_conv_forward_residual.argtypes = [vp, vp, fp, fp, fp, fp, fp, fp, fp, ctypes.c_int, fp, vp, ctypes.c_size_t]
    if hasattr(lib, "dau_conv_sigma_status"):            # (likewise: the device's record of the support each call's sigma needed)
        lib.dau_conv_sigma_status.argtypes = [vp] + [ctypes.POINTER(ctypes.c_int32)] * 3
    lib.dau_conv_last_status.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)]
    lib.dau_conv_filters.argtypes = [vp, vp, fp, fp]
    lib.dau_conv_unit_table.argtypes = [vp, vp, fp, fp, fp, ctypes.c_int, vp]
    lib.dau_conv_filter_support.argtypes = [ctypes.c_float]
    lib.dau_conv_filter_support.restype = ctypes.c_int
    lib.dau_conv_profile_begin.argtypes = [vp]
    lib.dau_conv_profile_end.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    if lib.dau_conv_abi_version() != 4:
        raise ImportError("dau_conv: ABI version mismatch in %s" % _LIB_PATH)
    return lib


lib = _load()


def filter_support(sigma):
    """k of the k x k prefilter for this sigma (2*ceil(5*sigma)+1 in float32): all a plan keeps of sigma_hint."""
    return int(lib.dau_conv_filter_support(ctypes.c_float(float(sigma))))


def build_id():
    """Fingerprint of the kernel sources the loaded library was built from (dau_conv_build_id)."""
    return lib.dau_conv_build_id().decode()


def _check(code):
    if code == DAU_OK:
        return
    msg = lib.dau_conv_last_error().decode("utf-8", "replace")
    raise {DAU_INVALID_ARGUMENT: InvalidArgumentError, DAU_FAILED_PRECONDITION: FailedPreconditionError}.get(
        code, InternalError)(msg)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    """The stream the library launches on: torch's current stream of the tensors' device (not of the current device)."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _same_device(*tensors):
    """All tensors of a call live on one GPU; returns it."""
    dev = tensors[0].device
    for t in tensors[1:]:
        if t is not None and t.device != dev:
            raise InvalidArgumentError("all tensors of a call must be on the same device (%s vs %s)" % (dev, t.device))
    return dev


def _req(t, name, shape=None, dtype=torch.float32, memory_format=torch.contiguous_format):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous(memory_format=memory_format)):
        raise InvalidArgumentError("%s must be a %s %s tensor on the GPU" % (
            name, "channels_last" if memory_format == torch.channels_last else "contiguous", str(dtype).replace("torch.", "")))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise InvalidArgumentError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t


# One grow-only workspace per (device, stream), shared by every plan: the layers of a network run one after the other on
# a stream, so they can reuse the same scratch memory (a north-star sized layer needs 3 GB for its backward pass).  The
# status word at the head of the workspace is read back by check_status() right after the call that wrote it.
# A call made while its stream is being captured into a graph stays out of it (Plan._workspace).
_SHARED_WS = {}


def capturing(device):
    """Is the current stream of this device being captured into a graph (torch.cuda.graph, make_graphed_callables, the cudagraph
    trees of torch.compile)?  False for a CPU device and before the GPU has been initialised."""
    if device.type != "cuda" or not torch.cuda.is_initialized():
        return False
    if device.index is None or device.index == torch.cuda.current_device():
        return torch.cuda.is_current_stream_capturing()
    with torch.cuda.device(device):
        return torch.cuda.is_current_stream_capturing()


def _pool_warmup(device):
    """Is this an ordinary call that the cudagraph trees of torch.compile make to warm a graph up?  They run it with the allocator
    already pointed at the graph's pool, and after it every tensor still alive in that pool must be an output of the graph: a shared
    workspace created or grown now would be such a tensor.  (Asked only when one would have to be; torch._inductor is not imported.)
    get_manager() and CUDAGraphTreeManager.in_warmup are internals of torch._inductor.cudagraph_trees, written against torch 2.10.  A
    torch without them is not warming up in a way this can see: tests/test_gpu_graph_capture.py's cudagraphs-backend test then fails on
    the trees' own check of their pool's live tensors.  Any other error is a real one and is raised."""
    trees = sys.modules.get("torch._inductor.cudagraph_trees")
    if trees is None:
        return False
    try:
        manager = trees.get_manager(device.index, create_if_none_exists=False)
        return manager is not None and bool(manager.in_warmup)
    except AttributeError:
        return False


# What a plan remembers of a forward / backward call: the workspace it kept (None: the call's own, gone with it), and whether the call
# was made under stream capture / as the warm-up of a graph's pool
_Call = collections.namedtuple("_Call", "ws captured transient")
_NO_CALL = _Call(None, False, False)


class Plan(object):
    """Owns one dau_conv_plan; scratch memory comes from the per-stream shared workspace.

    Streams and threads.  The dau_conv_plan itself is immutable, and one Plan is shared by every layer of a shape (the cache of
    dau_conv.py), so it may be called from several streams and host threads at once: each (device, stream) has a workspace of its
    own, and ctypes releases the GIL during a call.  What a Plan remembers of "the last call" -- `captured`, and the workspace whose
    status block check_status(), outlier_status(), line_status() and dot_line_status() read back -- is therefore kept per
    (device, stream), and every host thread asks about the stream of ITS most recent call: a thread that calls forward() and then
    check_status() gets the status of its own call, whatever other threads have enqueued on other streams in between.  The
    backward pass of autograd runs on a thread of torch's, on the stream of the forward call: it updates that stream's record, so
    the thread that called .backward() sees the backward call, as a single-threaded caller always did.  A thread that has made no
    call of its own is answered from the most recent call of any thread.  Two threads that call one plan on the SAME stream share
    that stream's workspace and record: the later call's status replaces the earlier one's, as with two calls of one thread.
    last_status() and sigma_status() read the plan's pinned mirror and belong to the plan, not to a stream."""

    def __init__(self, N, S, F, G, H, W, max_kernel_size=9, number_units_ignore=0, flags=FLAG_USE_INTERPOLATION,
                 algo=ALGO_AUTO, sigma_hint=0.5, mu_learning_rate_factor=1.0, device=None):
        d = _Desc(ctypes.sizeof(_Desc), N, S, F, G, H, W, int(max_kernel_size), int(number_units_ignore), int(flags),
                  int(algo), float(sigma_hint), float(mu_learning_rate_factor))
        self._h = ctypes.c_void_p()
        # a plan belongs to the device that is current when it is created (its kernels' launch attributes and its pinned
        # status mirror are set up there); `device` makes that explicit for callers whose current device is another one
        if device is not None and torch.cuda.is_available():
            with torch.cuda.device(device):
                _check(lib.dau_conv_plan_create(ctypes.byref(d), ctypes.byref(self._h)))
        else:
            _check(lib.dau_conv_plan_create(ctypes.byref(d), ctypes.byref(self._h)))
        self.N, self.S, self.F, self.G, self.H, self.W = N, S, F, G, H, W
        self.io_dtype = torch.bfloat16 if int(flags) & FLAG_IO_BF16 else torch.float16 if int(flags) & FLAG_IO_F16 else torch.float32
        # FLAG_IO_NHWC: activations of logical shape [N, C, H, W] with channels_last strides, in and out
        self._io_format = torch.channels_last if int(flags) & FLAG_IO_NHWC else torch.contiguous_format
        # FLAG_INPUT_RELU: forward() and backward() take the RAW input and compute relu(input) -> DAU and its gradients
        self.input_relu = bool(int(flags) & FLAG_INPUT_RELU)
        info = _Info()
        _check(lib.dau_conv_plan_get_info(self._h, ctypes.byref(info)))
        self.info = {n: getattr(info, n) for n, _ in _Info._fields_}
        self._ws = {}
        self._warm = set()           # devices on which an ordinary (not captured) call has completed: its launch attributes are set
        self._calls = {}             # (device index, stream handle) -> _Call: the most recent forward / backward call made there
        self._tls = threading.local()    # .key: where the calling thread made its most recent call; .pending: its call in the making
        self._any_key = None         # where any thread made the most recent call (for a thread that has made none)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:        # at interpreter shutdown the module globals may already be gone
            lib.dau_conv_plan_destroy(h)
            self._h = None

    def _call(self):
        """The record the calling thread asks about: of the stream of its own most recent call, else of any thread's."""
        return self._calls.get(getattr(self._tls, "key", None) or self._any_key, _NO_CALL)

    @property
    def captured(self):
        """The most recent forward / backward call (of this thread: see the class) was made under stream capture"""
        return self._call().captured

    @property
    def _transient(self):
        """... or as the warm-up of a graph whose pool must not keep its workspace (_pool_warmup)"""
        return self._call().transient

    @property
    def _last_ws(self):
        """The workspace that call kept (None: it kept none)"""
        return self._call().ws

    @property
    def io_layout(self):
        """"NHWC" for a FLAG_IO_NHWC plan (x, y, dy, dx are channels_last tensors), else "NCHW"."""
        return "NHWC" if self._io_format == torch.channels_last else "NCHW"

    def workspace_bytes(self, which):
        n = ctypes.c_size_t()
        _check(lib.dau_conv_workspace_bytes(self._h, which, ctypes.byref(n)))
        return n.value

    def _ws_bytes(self, which):
        """workspace_bytes(which), asked of the library once per plan and pass."""
        need = self._ws.get(which)
        if need is None:
            need = self._ws[which] = self.workspace_bytes(which)
        return need

    def _workspace(self, which, device):
        """The scratch memory of one pass (called with `device` current).  Under stream capture: a tensor of exactly the pass's size
        from the capturing allocator, which the caller drops when the call returns -- the graph's private pool hands memory out again
        in capture order, which is the order of the replay, so the pool holds the largest workspace of a model, not the sum; the
        shared workspace is neither read, grown nor replaced, and no pass reads what another left in its workspace."""
        need = self._ws_bytes(which)
        captured = torch.cuda.is_current_stream_capturing()
        key = (device.index, torch.cuda.current_stream(device).cuda_stream)
        self._tls.pending = (key, captured, False)       # (the calling thread's: the GIL is released during the library call)
        if captured:
            if device.index not in self._warm:
                # the first call of a plan on a device sets launch attributes behind a lock: not a stream operation
                raise FailedPreconditionError("DAUConv: this plan has made no call on %s yet; run the layer once before capturing "
                                              "(a plan's first call on a device sets its kernels' launch attributes)" % (device,))
            return torch.empty(max(need, 1), dtype=torch.uint8, device=device)
        shared = (device, key[1])
        ws = _SHARED_WS.get(shared)
        if ws is None or ws.numel() < need:
            if _pool_warmup(device):
                self._tls.pending = (key, False, True)   # a workspace of this call alone, as under capture: nothing of it outlives the call
                return torch.empty(max(need, 1), dtype=torch.uint8, device=device)
            ws = _SHARED_WS[shared] = torch.empty(need, dtype=torch.uint8, device=device)
        return ws

    def _called(self, ws, device):
        """A forward / backward call has been enqueued with this workspace (by the thread that asked _workspace for it)."""
        key, captured, transient = self._tls.pending
        # (the capture's workspace is not kept: it goes back to the graph's pool with the call)
        self._calls[key] = _Call(None if captured or transient else ws, captured, transient)
        self._tls.key = self._any_key = key
        if not captured:
            self._warm.add(device.index)

    def _status_ws(self, what):
        """The workspace whose status block the last call wrote, for the queries that read it back after the call."""
        call = self._call()          # (one look: another thread may make a call on the same stream while this one asks)
        if call.captured:
            raise FailedPreconditionError(
                "DAUConv: %s() reads the workspace of the plan's last call, and that call was captured into a graph (its workspace "
                "belongs to the graph's pool); ask last_status() / sigma_status(), which read the plan's pinned mirror" % what)
        if call.ws is None:
            raise FailedPreconditionError("DAUConv: %s() before any forward / backward call of this plan that kept its workspace" % what)
        return call.ws

    def _status_pair(self, what, query):
        """Sync; the pair of int32 that the library's `query` reads from the status block of the last call, for the method `what`."""
        a, b = ctypes.c_int32(), ctypes.c_int32()
        ws = self._status_ws(what)
        dev = ws.device
        with torch.cuda.device(dev):
            _check(getattr(lib, query)(self._h, _stream(dev), _ptr(ws), ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def epilogue_supported(self, epilogue=EPILOGUE_BIAS | EPILOGUE_RELU):
        """True if forward() takes this epilogue (EPILOGUE_* bits); raises InvalidArgumentError naming the reason otherwise: a plan
        whose forward pass runs on the direct kernels, a FLAG_DENSE_BF16 plan, unknown bits."""
        if not hasattr(lib, "dau_conv_epilogue_supported"):
            raise InvalidArgumentError("this build of the library has no fused epilogue")
        _check(lib.dau_conv_epilogue_supported(self._h, int(epilogue)))
        return True

    def _residual_supported(self):
        """True if forward() takes a residual: where it takes a bias.  Raises InvalidArgumentError naming the reason otherwise."""
        if not hasattr(lib, "dau_conv_forward_residual"):
            raise InvalidArgumentError("this build of the library has no fused residual")
        try:
            return self.epilogue_supported(EPILOGUE_BIAS)
        except InvalidArgumentError as e:
            raise InvalidArgumentError("no fused residual: %s" % e)

    def _req_call(self, x, dy=None, **params):
        """The checks every pass makes of its tensors, in this order: the input, the output gradient if the pass takes one, then the
        parameters as named -- each [1,S,G,F] float32."""
        _req(x, "input", (self.N, self.S, self.H, self.W), self.io_dtype, self._io_format)
        if dy is not None:
            _req(dy, "grad", (self.N, self.F, self.H, self.W), self.io_dtype, self._io_format)
        for name, t in params.items():
            _req(t, name, (1, self.S, self.G, self.F))

    def _new_grads(self, need_mask, dev):
        """(dw, dmu1, dmu2, dsigma): a fresh [1,S,G,F] float32 tensor for each one need_mask asks for, None for the others."""
        return tuple(torch.empty((1, self.S, self.G, self.F), dtype=torch.float32, device=dev) if need_mask & bit else None
                     for bit in (NEED_DW, NEED_DMU1, NEED_DMU2, NEED_DSIGMA))

    def forward(self, x, w, mu1, mu2, sigma, bias=None, relu=False, residual=None):
        """y, or with bias ([F] float32) / residual / relu the fused epilogue y = act((sum + bias[f]) + residual[n,f,h,w]): fp32 adds
        in that order and a clamp on the value the plain call stores, before the store's one rounding; y keeps the plan's dtype and
        layout.  residual: a tensor like y (shape, dtype, layout) that is only read; it must not share memory with anything the call
        writes.  A residual without bias or relu is a plain fused add."""
        if residual is not None:             # (first: a plan that takes none is refused whatever the tensors are)
            self._residual_supported()
            yshape = (self.N, self.F, self.H, self.W)
            if tuple(residual.shape) != yshape:      # (the shape before the device: a refusal that names the shape wherever the tensor lives)
                raise InvalidArgumentError("residual has shape %s, expected %s" % (tuple(residual.shape), yshape))
            _req(residual, "residual", yshape, self.io_dtype, self._io_format)
        self._req_call(x, weights=w, mu1=mu1, mu2=mu2, sigma=sigma)
        if bias is not None:
            _req(bias, "bias", (self.F,))
        dev = _same_device(x, w, mu1, mu2, sigma, bias, residual)
        epilogue = (EPILOGUE_BIAS if bias is not None else 0) | (EPILOGUE_RELU if relu else 0)
        if epilogue:
            self.epilogue_supported(epilogue)
        # the library launches on the CURRENT device: make that the tensors' device for the duration of the call
        with torch.cuda.device(dev):
            y = torch.empty((self.N, self.F, self.H, self.W), dtype=self.io_dtype, device=dev, memory_format=self._io_format)
            ws = self._workspace(PASS_FORWARD, dev)
            if residual is not None:
                _check(lib.dau_conv_forward_residual(self._h, _stream(dev), _ptr(x), _ptr(w), _ptr(mu1), _ptr(mu2), _ptr(sigma),
                                                     _ptr(bias) if bias is not None else None, _ptr(residual), epilogue, _ptr(y),
                                                     _ptr(ws), ws.numel()))
            elif epilogue:
                _check(lib.dau_conv_forward_epilogue(self._h, _stream(dev), _ptr(x), _ptr(w), _ptr(mu1), _ptr(mu2), _ptr(sigma),
                                                     _ptr(bias), epilogue, _ptr(y), _ptr(ws), ws.numel()))
            else:
                _check(lib.dau_conv_forward(self._h, _stream(dev), _ptr(x), _ptr(w), _ptr(mu1), _ptr(mu2), _ptr(sigma), _ptr(y),
                                            _ptr(ws), ws.numel()))
        self._called(ws, dev)
        return y

    def epilogue_backward(self, dy, y=None, relu=False, need_dbias=True, dz=None):
        """Backward of forward()'s epilogue -> (dz, dbias).  relu: dz = (y <= 0) ? 0 : dy from the stored y, in dy's dtype and
        layout, written into `dz` if given (it may be dy itself); without relu dz is None -- the gradient of the sum IS dy, nothing
        is copied.  dbias = dz (or dy) summed over n, h, w: [F] float32, fixed summation order, None unless need_dbias.
        The caller passes dz (or dy) on to backward() / backward_param_sums()."""
        shape = (self.N, self.F, self.H, self.W)
        _req(dy, "grad", shape, self.io_dtype, self._io_format)
        if relu:
            if y is None:
                raise InvalidArgumentError("epilogue_backward(relu=True) needs the stored y")
            _req(y, "output", shape, self.io_dtype, self._io_format)
            if dz is not None:
                _req(dz, "dz", shape, self.io_dtype, self._io_format)
        dev = _same_device(dy, y if relu else None, dz if relu else None)
        epilogue = (EPILOGUE_BIAS if need_dbias else 0) | (EPILOGUE_RELU if relu else 0)
        if not epilogue:
            return None, None
        with torch.cuda.device(dev):
            if relu and dz is None:
                dz = torch.empty(shape, dtype=self.io_dtype, device=dev, memory_format=self._io_format)
            dbias = torch.empty((self.F,), dtype=torch.float32, device=dev) if need_dbias else None
            # a small workspace of its own: the shared one still holds the status block of the last forward / backward call
            need = self._ws_bytes(PASS_EPILOGUE_BACKWARD)
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev) if need_dbias else None
            _check(lib.dau_conv_epilogue_backward(self._h, _stream(dev), _ptr(dy), _ptr(y) if relu else None, epilogue,
                                                  _ptr(dz) if relu else None, _ptr(dbias), _ptr(ws), need if need_dbias else 0))
        return (dz if relu else None), dbias

    def backward(self, x, dy, w, mu1, mu2, sigma, need_mask=NEED_ALL):
        self._req_call(x, dy, weights=w, mu1=mu1, mu2=mu2, sigma=sigma)
        dev = _same_device(x, dy, w, mu1, mu2, sigma)
        with torch.cuda.device(dev):
            dx = torch.empty(x.shape, dtype=self.io_dtype, device=dev, memory_format=self._io_format) if need_mask & NEED_DX else None
            dw, dmu1, dmu2, dsigma = self._new_grads(need_mask, dev)
            ws = self._workspace(PASS_BACKWARD, dev)
            _check(lib.dau_conv_backward(self._h, _stream(dev), _ptr(x), _ptr(dy), _ptr(w), _ptr(mu1), _ptr(mu2), _ptr(sigma),
                                         _ptr(dx), _ptr(dw), _ptr(dmu1), _ptr(dmu2), _ptr(dsigma), _ptr(ws), ws.numel(),
                                         int(need_mask)))
        self._called(ws, dev)
        return dx, dw, dmu1, dmu2, dsigma

    def backward_param_sums(self, x, dy, mu1, mu2, sigma, out=None):
        """Raw parameter-gradient sums [4, S, G, F] (kinds w, mu1, mu2, sigma) of this batch: linear in the batch, so a
        data-parallel caller all-reduces THIS buffer and only then calls finalize_param_grads()."""
        self._req_call(x, dy, mu1=mu1, mu2=mu2, sigma=sigma)
        dev = _same_device(x, dy, mu1, mu2, sigma, out)
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty((4, self.S, self.G, self.F), dtype=torch.float32, device=dev)
            _req(out, "sums", (4, self.S, self.G, self.F))
            ws = self._workspace(PASS_BACKWARD, dev)
            _check(lib.dau_conv_backward_param_sums(self._h, _stream(dev), _ptr(x), _ptr(dy), _ptr(mu1), _ptr(mu2), _ptr(sigma),
                                                    _ptr(out), _ptr(ws), ws.numel()))
        self._called(ws, dev)
        return out

    def finalize_param_grads(self, sums, w, need_mask=NEED_DW | NEED_DMU1 | NEED_DMU2 | NEED_DSIGMA):
        """(dw, dmu1, dmu2, dsigma) from (all-reduced) sums: dmu *= w * lr, dsigma *= w, ignored units -> 0, NaN dmu -> 0."""
        _req(sums, "sums", (4, self.S, self.G, self.F))
        _req(w, "weights", (1, self.S, self.G, self.F))
        dev = _same_device(sums, w)
        with torch.cuda.device(dev):
            dw, dmu1, dmu2, dsigma = self._new_grads(need_mask, dev)
            _check(lib.dau_conv_finalize_param_grads(self._h, _stream(dev), _ptr(sums), _ptr(w), _ptr(dw), _ptr(dmu1),
                                                     _ptr(dmu2), _ptr(dsigma), int(need_mask)))
        return dw, dmu1, dmu2, dsigma

    def check_status(self):
        """Sync + raise if the last call saw NaN or out-of-bucket offsets; returns max(|mu|)."""
        mx = ctypes.c_float()
        ws = self._status_ws("check_status")
        dev = ws.device
        with torch.cuda.device(dev):
            _check(lib.dau_conv_check_status(self._h, _stream(dev), _ptr(ws), ctypes.byref(mx)))
        return mx.value

    def outlier_status(self):
        """Sync; -> (outlier_units, ring_taken) of the last call: the live units with max(|mu1|,|mu2|) > 3, and whether one of its
        gather-sum passes ran as the radius-3 GEMM plus the ring pass (FLAG_DENSE_SPLIT_OUTLIERS) rather than another member."""
        units, taken = self._status_pair("outlier_status", "dau_conv_gather_outlier_status")
        return units, bool(taken)

    def split_dot_geometry(self):
        """-> (region_width, strip_items, strip_k_steps) of the two-limb f16 parameter-gradient kernel: the K steps of a full item,
        the items of one column strip and the K steps the kernel runs for a strip (a strip's last item takes ceil(region_width / 4)
        where (H + 1) % 4 == 1); zeros for a plan without that kernel.  No device needed."""
        v = [ctypes.c_int32() for _ in range(3)]
        _check(lib.dau_conv_split_dot_geometry(self._h, *[ctypes.byref(c) for c in v]))
        return tuple(c.value for c in v)

    def line_status(self):
        """Sync; -> (off_line_units, line_radius_taken) of the last call: the units of its gather-sum table that do not lie on the row
        of their pixel (counted by plans that hold a line member, FLAG_DENSE_SPLIT_LINE), and 4 or 8 if its gather-sum pass ran as the
        line member of that radius, 0 if another member did the work."""
        return self._status_pair("line_status", "dau_conv_gather_line_status")

    def dot_line_status(self):
        """Sync; -> (off_line_units, line_radius_taken) of the last backward call: the units of its bare parameter-gradient table that
        do not lie on the row of their pixel (counted by plans that hold a line member of the gather-dot, FLAG_SPLIT_DOT_LINE), and
        4 or 8 if its parameter gradients ran as the line member of that radius, 0 if another member did the work."""
        return self._status_pair("dot_line_status", "dau_conv_dot_line_status")

    def last_status(self):
        """No sync: max(|mu|) seen by the most recent COMPLETED call of this plan (None before any has completed);
        raises if that call saw NaN or out-of-bucket offsets.  Calling it before every op call surfaces a bad offset
        one call late without ever stalling the stream."""
        mx, valid = ctypes.c_float(), ctypes.c_int32()
        _check(lib.dau_conv_last_status(self._h, ctypes.byref(mx), ctypes.byref(valid)))
        return mx.value if valid.value else None

    def sigma_status(self):
        """No sync: (needed, planned, worst_needed) prefilter supports.  planned: the plan's k (2*ceil(5*sigma_hint)+1); needed: what the
        sigma of the most recent call asked for, as the device recorded it (0: non-finite or not positive; 19: beyond 17); worst_needed:
        the largest `needed` above `planned` since this was last asked -- sticky, cleared by this call; 0: none.  A graph replay runs
        no Python, so a sigma trained across a support boundary shows up here (dau_conv.check_pending_offsets() raises for it)."""
        if not hasattr(lib, "dau_conv_sigma_status"):
            return 0, self.info["blur_support"], 0
        v = [ctypes.c_int32() for _ in range(3)]
        _check(lib.dau_conv_sigma_status(self._h, *[ctypes.byref(c) for c in v]))
        return tuple(c.value for c in v)

    def profile_begin(self):
        _check(lib.dau_conv_profile_begin(self._h))

    def profile_end(self):
        """-> {slot name: (summed ms of the dominant kernel's launches, passes they made up)} since profile_begin()."""
        ms = (ctypes.c_double * 3)()
        n = (ctypes.c_int32 * 3)()
        _check(lib.dau_conv_profile_end(self._h, ms, n))
        return {name: (ms[i], n[i]) for i, name in enumerate(("gather_sum_fwd", "gather_sum_dx", "gather_dot"))}

    def filters(self, sigma):
        k = self.info["blur_support"]
        out = torch.empty((6, k, k), dtype=torch.float32, device=sigma.device)
        with torch.cuda.device(sigma.device):
            _check(lib.dau_conv_filters(self._h, _stream(sigma.device), _ptr(sigma), _ptr(out)))
        return out

    def unit_table(self, mu1, mu2, w=None, form=0):
        """The table the gather kernels consume, from the kernel every call runs first: -> (offsets int32 [units, 2],
        factors float32 [units, 4]).  form 0: [S][G][F] order (w=None: bare factors, the parameter-gradient pass);
        form 1: [F][G][S] order with negated offsets (the input-gradient pass)."""
        units = self.S * self.G * self.F
        raw = torch.empty((units, 6), dtype=torch.int32, device=mu1.device)
        with torch.cuda.device(mu1.device):
            _check(lib.dau_conv_unit_table(self._h, _stream(mu1.device), _ptr(w), _ptr(mu1), _ptr(mu2), int(form), _ptr(raw)))
        return raw[:, :2].contiguous(), raw[:, 2:].contiguous().view(torch.float32)
