"""CPU: the two opaque ops behind the torch.compile path (dau_conv/_ops.py) -- that they are registered by `import dau_conv` without
touching the GPU, and that their shape functions are pure: on fake CUDA tensors (no device needed) they give the promised shape,
dtype and strides of y and of every gradient, create no plan, and keep a symbolic batch symbolic."""
import itertools
import sys

import pytest
import torch

S, G, F, N, H, W = 4, 4, 8, 2, 8, 9
_SETTINGS = dict(number_units_ignore=0, kernel_size=9, unit_testing=False, mu_learning_rate_factor=1.0, single_dim_kernel=False,
                 forbid_positive_dim1=False, use_interpolation=True, algo=0, dense_bf16=False, dense_split=-1, dense_outliers=False,
                 channels_last=-1, check_offsets="async")
_ORDER = ("number_units_ignore", "kernel_size", "unit_testing", "mu_learning_rate_factor", "single_dim_kernel", "forbid_positive_dim1",
          "use_interpolation", "algo", "dense_bf16", "dense_split", "dense_outliers", "channels_last", "check_offsets")
NEED_DX, NEED_ALL = 1, 31


def _settings(**kw):
    st = dict(_SETTINGS, **kw)
    return tuple(st[k] for k in _ORDER)


def _strides(shape, nhwc):
    n, c, h, w = shape
    return (h * w * c, 1, w * c, c) if nhwc else (c * h * w, h * w, w, 1)


def _fake_inputs(dtype, channels_last_input, n=N):
    x = torch.empty(n, S, H, W, device="cuda", dtype=dtype)
    if channels_last_input:
        x = x.contiguous(memory_format=torch.channels_last)
    p = [torch.empty(1, S, G, F, device="cuda") for _ in range(3)]
    sigma = torch.empty(1, device="cuda")
    return x, p, sigma


def test_import_registers_both_ops_and_leaves_the_gpu_alone():
    # (in this process another test may have used the GPU already: unchanged here, strictly "not initialised" in the fresh
    # interpreter of test_import_does_not_pull_in_dynamo)
    was = torch.cuda.is_initialized()
    import dau_conv  # noqa: F401
    assert torch.cuda.is_initialized() == was
    for name in ("conv", "conv_backward"):
        op = getattr(torch.ops.dau_conv, name).default
        schema = op._schema
        assert not schema.is_mutable, schema
        assert all(a.alias_info is None for a in schema.arguments), schema
    conv = torch.ops.dau_conv.conv.default._schema
    assert [a.name for a in conv.arguments][:9] == ["x", "w", "mu1", "mu2", "sigma", "bias", "residual", "relu", "input_relu"]
    assert tuple(a.name for a in conv.arguments[9:]) == _ORDER
    back = torch.ops.dau_conv.conv_backward.default._schema
    assert [a.name for a in back.arguments][:11] == ["grad", "x", "w", "mu1", "mu2", "sigma", "y", "relu", "input_relu", "need_mask",
                                                     "need_dbias"]
    assert tuple(a.name for a in back.arguments[11:]) == _ORDER and len(back.returns) == 6
    assert torch.cuda.is_initialized() == was


# _settings() keywords per trailing argument of the ops: every value the argument takes, the packed pairs in full (dense_line rides
# in dense_split, dense_line_grads in algo; both need a single-dimension layer)
_ROUND_TRIP = {
    "number_units_ignore": [dict(number_units_ignore=v) for v in (0, 1, 3)],
    "kernel_size": [dict(kernel_size=v) for v in (9, 17, 33)],
    "unit_testing": [dict(unit_testing=v) for v in (False, True)],
    "mu_learning_rate_factor": [dict(mu_learning_rate_factor=v) for v in (1.0, 500.0, 0.25)],
    "single_dim_kernel": [dict(single_dim_kernel=v) for v in (False, True)],
    "forbid_positive_dim1": [dict(forbid_positive_dim1=v) for v in (False, True)],
    "use_interpolation": [dict(use_interpolation=v) for v in (True, False)],
    "algo": [dict(algo=a, dense_line_grads=g, single_dim_kernel=g) for a in (0, 1, 2) for g in (False, True)],
    "dense_bf16": [dict(dense_bf16=v) for v in (False, True)],
    "dense_split": [dict(dense_split=s, dense_line=line, single_dim_kernel=line)
                    for s, line in ((None, False), (False, False), (True, False), (None, True), (True, True))],
    "dense_outliers": [dict(dense_outliers=v) for v in (False, True)],
    "channels_last": [dict(channels_last=v) for v in (None, False, True)],
    "check_offsets": [dict(check_offsets=v) for v in ("async", True, False)],
}


@pytest.mark.parametrize("name", _ORDER)
def test_settings_round_trip_through_the_ops_arguments(name):
    """_run_settings(w, sigma, False, *encode_settings(st)) gives st back, key for key and type for type, for every value of every
    trailing argument; the values of an argument all encode differently, and only in that argument's slot."""
    import importlib
    from dau_conv import _ops
    impl = importlib.import_module("dau_conv.dau_conv")
    assert tuple(s.name for s in _ops._SETTINGS) == _ORDER == tuple(_ROUND_TRIP) and _ops._N_ARGS == 9 + len(_ORDER)
    sigma, w = torch.full((1,), 0.5), torch.zeros(1, S, G, F)
    plain = _ops.encode_settings(impl._settings(sigma, num_output=F))
    slot, seen = _ORDER.index(name), set()
    for kw in _ROUND_TRIP[name]:
        st = impl._settings(sigma, num_output=F, **kw)
        enc = _ops.encode_settings(st)
        assert len(enc) == len(_ORDER)
        # (single_dim_kernel, which the line options need, has a slot of its own)
        assert all(enc[i] == plain[i] for i in range(len(enc)) if i != slot and _ORDER[i] != "single_dim_kernel"), (kw, enc)
        seen.add(enc[slot])
        back = _ops._run_settings(w, sigma, False, *enc)
        assert back == st and all(type(back[k]) is type(st[k]) for k in st), (kw, back, st)
        assert _ops._run_settings(w, sigma, True, *enc) == dict(st, input_relu=True)
    assert len(seen) == len(_ROUND_TRIP[name])


def test_import_does_not_pull_in_dynamo():
    import subprocess
    code = ("import sys; sys.path[:0] = %r; import dau_conv, torch; "
            "assert 'torch._dynamo' not in sys.modules; assert not torch.cuda.is_initialized(); "
            "assert torch.ops.dau_conv.conv is not None") % ([p for p in sys.path if p],)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)


@pytest.mark.parametrize("epilogue", list(itertools.product([False, True], repeat=3)),
                         ids=lambda e: "bias%d_relu%d_res%d" % tuple(int(v) for v in e))
@pytest.mark.parametrize("channels_last", [-1, 1, 0], ids=["cl_none", "cl_true", "cl_false"])
@pytest.mark.parametrize("channels_last_input", [False, True], ids=["contiguous", "channels_last"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["float32", "float16", "bfloat16"])
def test_fake_propagation(dtype, channels_last_input, channels_last, epilogue):
    import importlib
    import dau_conv  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    impl = importlib.import_module("dau_conv.dau_conv")
    plans_before = dict(impl._PLANS)                     # (empty in a process that has run no plan)
    with_bias, relu, with_res = epilogue
    nhwc = channels_last_input and channels_last != 0        # (every dtype runs the NHWC plan by default: _NHWC_BY_DEFAULT)
    st = _settings(channels_last=channels_last)
    with FakeTensorMode():
        x, (w, mu1, mu2), sigma = _fake_inputs(dtype, channels_last_input)
        bias = torch.empty(F, device="cuda") if with_bias else None
        res = torch.empty(N, F, H, W, device="cuda", dtype=dtype) if with_res else None
        y = torch.ops.dau_conv.conv(x, w, mu1, mu2, sigma, bias, res, relu, False, *st)
        assert tuple(y.shape) == (N, F, H, W) and y.dtype == dtype and y.device.type == "cuda"
        assert tuple(y.stride()) == _strides((N, F, H, W), nhwc)
        y_in = torch.ops.dau_conv.conv(x, w, mu1, mu2, sigma, bias, res, relu, True, *st)           # the input ReLU changes nothing
        assert (y_in.shape, y_in.dtype, y_in.stride()) == (y.shape, y.dtype, y.stride())
        grad = torch.empty_like(y)
        for need, need_dbias in ((NEED_ALL, with_bias), (NEED_DX, False), (NEED_ALL & ~NEED_DX, with_bias)):
            out = torch.ops.dau_conv.conv_backward(grad, x, w, mu1, mu2, sigma, y if relu else None, relu, False, need, need_dbias, *st)
            assert len(out) == 6
            dx, params, dbias = out[0], out[1:5], out[5]
            assert dx.dtype == dtype
            if need & NEED_DX:
                assert tuple(dx.shape) == (N, S, H, W) and tuple(dx.stride()) == _strides((N, S, H, W), nhwc)
            else:
                assert dx.numel() == 0
            for g in params:
                assert g.dtype == torch.float32
                if need & ~NEED_DX:
                    assert tuple(g.shape) == (1, S, G, F) and g.is_contiguous()
                else:
                    assert g.numel() == 0
            assert dbias.dtype == torch.float32
            assert (tuple(dbias.shape) == (F,)) if need_dbias else (dbias.numel() == 0)
        # single gradients: only the one asked for has elements
        for i, bit in enumerate((2, 4, 8, 16)):
            out = torch.ops.dau_conv.conv_backward(grad, x, w, mu1, mu2, sigma, y if relu else None, relu, False, bit, False, *st)
            assert [int(g.numel() > 0) for g in out] == [0] + [int(j == i) for j in range(4)] + [0]
    assert dict(impl._PLANS) == plans_before, "a shape function created a plan"
    # (where a device is visible, making a fake CUDA tensor initialises the GPU by itself: nothing to assert about that here)


def test_fake_dense_bf16_keeps_bfloat16_contiguous():
    """DAU_FLAG_IO_NHWC excludes DAU_FLAG_DENSE_BF16: a channels_last bfloat16 input of such a layer gets a contiguous output, even
    with channels_last=True; float16 input of the same layer is not affected."""
    import dau_conv  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        for dtype, nhwc in ((torch.bfloat16, False), (torch.float16, True)):
            x, (w, mu1, mu2), sigma = _fake_inputs(dtype, True)
            st = _settings(dense_bf16=True, channels_last=1)
            y = torch.ops.dau_conv.conv(x, w, mu1, mu2, sigma, None, None, False, True, *st)
            assert tuple(y.stride()) == _strides((N, F, H, W), nhwc) and y.dtype == dtype
            dx = torch.ops.dau_conv.conv_backward(y, x, w, mu1, mu2, sigma, None, False, True, NEED_DX, False, *st)[0]
            assert tuple(dx.stride()) == _strides((N, S, H, W), nhwc)


def test_fake_full_sigma_tensor_and_half_parameters():
    """sigma may be the full [1,S,G,F] tensor, and the parameters of any floating dtype: the gradients stay float32."""
    import dau_conv  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x, (w, mu1, mu2), _ = _fake_inputs(torch.float16, False)
        w, mu1, mu2 = w.half(), mu1.half(), mu2.half()
        sigma = torch.empty(1, S, G, F, device="cuda", dtype=torch.float16)
        y = torch.ops.dau_conv.conv(x, w, mu1, mu2, sigma, None, None, False, False, *_settings())
        out = torch.ops.dau_conv.conv_backward(y, x, w, mu1, mu2, sigma, None, False, False, NEED_ALL, False, *_settings())
        assert all(g.dtype == torch.float32 and tuple(g.shape) == (1, S, G, F) for g in out[1:5])


@pytest.mark.parametrize("channels_last_input", [False, True], ids=["contiguous", "channels_last"])
def test_symbolic_batch_stays_symbolic(channels_last_input):
    import importlib
    import dau_conv  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import DimDynamic, ShapeEnv, StatelessSymbolicContext
    impl = importlib.import_module("dau_conv.dau_conv")
    plans_before = dict(impl._PLANS)
    shape_env = ShapeEnv()
    mode = FakeTensorMode(shape_env=shape_env)
    real = torch.empty(N, S, H, W)
    if channels_last_input:
        real = real.contiguous(memory_format=torch.channels_last)
    x = mode.from_tensor(real, symbolic_context=StatelessSymbolicContext(
        dynamic_sizes=[DimDynamic.DYNAMIC, DimDynamic.STATIC, DimDynamic.STATIC, DimDynamic.STATIC]))
    assert isinstance(x.shape[0], torch.SymInt)
    with mode:
        w, mu1, mu2 = (torch.empty(1, S, G, F) for _ in range(3))
        sigma = torch.empty(1)
        bias = torch.empty(F)
        y = torch.ops.dau_conv.conv(x, w, mu1, mu2, sigma, bias, None, True, True, *_settings())
        assert isinstance(y.shape[0], torch.SymInt) and y.shape[0] == x.shape[0] and tuple(y.shape[1:]) == (F, H, W)
        assert tuple(y.stride()) == _strides((N, F, H, W), channels_last_input)
        out = torch.ops.dau_conv.conv_backward(torch.empty_like(y), x, w, mu1, mu2, sigma, y, True, True, NEED_ALL, True, *_settings())
        assert isinstance(out[0].shape[0], torch.SymInt) and tuple(out[0].shape[1:]) == (S, H, W)
        assert tuple(out[0].stride()) == _strides((N, S, H, W), channels_last_input)
        assert tuple(out[1].shape) == (1, S, G, F) and tuple(out[5].shape) == (F,)
    # nothing pinned the batch to the example's value
    assert not any("Eq(s" in str(g.expr) for g in shape_env.guards), shape_env.guards
    assert dict(impl._PLANS) == plans_before


def _tracing_backend(graphs):
    """a backend that keeps the graph Dynamo hands it and answers with zeros of the traced shapes: tracing needs no device"""
    def backend(gm, example_inputs):
        graphs.append(gm)
        outs = [n for n in gm.graph.nodes if n.op == "output"][0].args[0]
        return lambda *a: [torch.zeros([int(v) for v in o.meta["example_value"].shape], dtype=o.meta["example_value"].dtype)
                           for o in outs]
    return backend


@pytest.mark.parametrize("kw", [dict(), dict(dau_sigma_trainable=True), dict(fused_epilogue=True, activation=torch.relu, strides=2),
                                dict(input_activation="relu", channels_last=True)],
                         ids=["default", "sigma_trainable", "fused_strided", "input_relu"])
def test_a_layer_traces_into_one_graph_with_one_dau_op(kw):
    """Dynamo traces DAUConv2d.forward end to end (fullgraph=True) on CPU tensors: one graph, one dau_conv.conv node, no .item() --
    sigma goes into the op as it is -- and an in-place write of sigma does not trace again."""
    import warnings
    import dau_conv
    import torch._dynamo
    torch._dynamo.reset()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        layer = dau_conv.DAUConv2d(filters=F, dau_units=(2, 2), max_kernel_size=9, in_channels=S, **kw)
    graphs = []
    compiled = torch.compile(layer, backend=_tracing_backend(graphs), fullgraph=True)
    x = torch.randn(N, S, H, W)
    with torch.no_grad():
        y = compiled(x)
        assert tuple(y.shape) == ((N, F, 4, 5) if kw.get("strides") == 2 else (N, F, H, W))
        layer.sigma.fill_(0.61)
        compiled(x)
    assert len(graphs) == 1
    targets = [str(n.target) for n in graphs[0].graph.nodes if n.op in ("call_function", "call_method")]
    assert sum("dau_conv.conv" in t for t in targets) == 1, targets
    assert not any("item" in t and "getitem" not in t for t in targets), targets
    sigma_args = [n for n in graphs[0].graph.nodes if "dau_conv.conv" in str(n.target)][0].args[4]
    assert tuple(sigma_args.meta["example_value"].shape) == (1,), "sigma reaches the op untiled"
    torch._dynamo.reset()


def test_process_group_layer_is_refused_by_fullgraph_by_name():
    import dau_conv
    import torch._dynamo
    torch._dynamo.reset()
    layer = dau_conv.DAUConv2d(filters=F, dau_units=(2, 2), max_kernel_size=9, in_channels=S, process_group=True)
    with pytest.raises(Exception, match="process_group"):
        torch.compile(layer, backend=_tracing_backend([]), fullgraph=True)(torch.randn(N, S, H, W))
    torch._dynamo.reset()
