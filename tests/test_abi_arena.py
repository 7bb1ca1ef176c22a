"""CPU: tests/abi_arena.py itself, so that a canary report of test_gpu_memory_contract.py can be trusted.  The carving arithmetic
(offsets, canary bands, skew, alignment) is a pure function of the buffer sizes; the two 16-bit storage conversions; and the
harness's bookkeeping end to end in host memory, against a stand-in for the library that writes exactly what it is told to: a
well-behaved call is reported clean, and an overrun of an output, of the workspace or of an input, a changed input and a write
to an output that was not requested are each reported as what they are."""
import ctypes

import numpy as np
import pytest

import abi_arena as aa


def _sizes(N, S, F, G, H, W, esize, ws, sums=True):
    units = S * G * F
    sizes = dict(x=N * S * H * W * esize, dy=N * F * H * W * esize, y=N * F * H * W * esize, dx=N * S * H * W * esize, workspace=ws)
    for n in ("w", "mu1", "mu2", "sigma", "dw", "dmu1", "dmu2", "dsigma"):
        sizes[n] = 4 * units
    if sums:
        sizes["sums"] = 16 * units
    return sizes


SHAPES = [(3, 5, 9, 3, 13, 21), (2, 7, 5, 2, 9, 8), (1, 1, 1, 1, 1, 1), (2, 33, 130, 2, 12, 12)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("esize", [4, 2])
@pytest.mark.parametrize("skew", [0, 1, 3])
@pytest.mark.parametrize("ws", [16, 4097, 1234567])
def test_layout(shape, esize, skew, ws):
    sizes = _sizes(*shape, esize=esize, ws=ws, sums=ws != 16)
    lay = aa.layout(sizes, esize, skew)
    assert list(lay.regions) == [n for n in aa.ORDER if n in sizes]
    # regions and bands tile the arena without gap or overlap, alternating band / region, a band at either end
    pieces = sorted(list(lay.regions.values()) + lay.bands, key=lambda r: r.offset)
    assert pieces[0].offset == 0 and pieces[-1].offset + pieces[-1].size == lay.total
    for a, b in zip(pieces, pieces[1:]):
        assert a.offset + a.size == b.offset, (a, b)
        assert (a in lay.bands) != (b in lay.bands), (a, b)
    assert pieces[0] in lay.bands and pieces[-1] in lay.bands and len(lay.bands) == len(lay.regions) + 1
    for b in lay.bands:
        assert b.size >= 1 << 20, b
        assert b.size < (1 << 20) + aa.ALIGN + skew * esize      # (and no larger than alignment and skew make it)
    for n, r in lay.regions.items():
        assert r.size == sizes[n]
        if n in aa.ACTIVATIONS:
            assert r.offset % aa.ALIGN == skew * esize, (n, r)
        else:
            assert r.offset % aa.ALIGN == 0, (n, r)
    assert lay.regions["workspace"].offset % 256 == 0


def test_skew_one_defeats_every_alignment_switch():
    """skew 1: base % 16 == 4 for fp32 (no 16-byte loads), base % 8 == 2 for the 16-bit formats (no 8- or 16-byte loads)"""
    for esize, mod, want in ((4, 16, 4), (2, 8, 2), (2, 16, 2)):
        lay = aa.layout(_sizes(3, 5, 9, 3, 13, 21, esize=esize, ws=1000), esize, 1)
        for n in aa.ACTIVATIONS:
            assert lay.regions[n].offset % mod == want, (esize, n)
        for n in ("w", "mu1", "mu2", "sigma", "dw", "sums", "workspace"):
            assert lay.regions[n].offset % 256 == 0
    lay = aa.layout(_sizes(3, 5, 9, 3, 13, 21, esize=4, ws=1000), 4, 0)
    assert all(r.offset % 256 == 0 for r in lay.regions.values())


def test_buffers_that_a_call_lacks_get_no_region():
    sizes = _sizes(2, 3, 4, 1, 5, 5, esize=4, ws=64, sums=False)
    lay = aa.layout(sizes, 4)
    assert "sums" not in lay.regions and [b.name for b in lay.bands][-1] == "after_workspace"
    assert lay.bands[-2].name == "before_workspace" and lay.bands[-3].name == "before_dsigma"


def test_layout_is_a_pure_function():
    sizes = _sizes(2, 7, 5, 2, 9, 6, esize=2, ws=99999)
    assert aa.layout(dict(sizes), 2, 1) == aa.layout(dict(sizes), 2, 1)


def test_storage_round_trips():
    rs = np.random.RandomState(0)
    a = np.concatenate([rs.randn(1000), rs.randn(1000) * 1e-6, [0.0, -0.0, 1.0, 65504.0, 2.0 ** -24]]).astype(np.float32)
    assert aa.widen(aa.to_storage(a, "f32"), "f32") is not None and np.array_equal(aa.to_storage(a, "f32"), a)
    h = aa.to_storage(a, "f16")
    assert h.dtype == np.uint16 and np.array_equal(aa.widen(h, "f16"), a.astype(np.float16).astype(np.float32))
    b = aa.to_storage(a, "bf16")
    back = aa.widen(b, "bf16")
    assert b.dtype == np.uint16 and np.array_equal(aa.to_storage(back, "bf16"), b)            # bf16 values are fixed points
    assert np.all(np.abs(back - a) <= np.abs(a) * 2.0 ** -8)                                    # half an ulp of 8 significant bits
    tie = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)                          # ties go to the even neighbour
    assert np.array_equal(aa.widen(aa.to_storage(tie, "bf16"), "bf16"), np.array([1.0, 1.0 + 2.0 ** -6], np.float32))
    import torch
    assert np.array_equal(aa.to_storage(a, "bf16"), torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    # the three poison fills: NaN / huge but finite
    for io, dt in (("f32", np.uint32), ("f16", np.uint16), ("bf16", np.uint16)):
        nan = np.frombuffer(b"\xff" * 8, dtype=dt)
        big = np.frombuffer(b"\x7b" * 8, dtype=dt)
        v = aa.widen(nan.view(np.float32) if io == "f32" else nan, io)
        assert np.isnan(v).all()
        v = aa.widen(big.view(np.float32) if io == "f32" else big, io)
        assert np.isfinite(v).all() and (v > 6e4).all()


# ---- the harness itself, in host memory: a stand-in for the library that writes what it is told to, so that every kind of damage the
# ---- GPU tests rely on the harness to report is shown to be reported
class _StandIn(object):
    """The five entry points the harness calls, over host memory.  Writes zeros into the outputs a call requests and into the status
    block; `damage` = (buffer name, byte offset relative to the buffer's END, bytes) adds one stray write per forward call."""

    def __init__(self, capi, plan, esize):
        self.capi, self.plan, self.damage, self.stray = capi, plan, None, {}
        units = plan.S * plan.G * plan.F
        self.ybytes, self.xbytes, self.pbytes = plan.N * plan.F * plan.H * plan.W * esize, plan.N * plan.S * plan.H * plan.W * esize, 4 * units

    @staticmethod
    def _zero(p, n):
        if p is not None:
            ctypes.memset(p.value if hasattr(p, "value") else p, 0, n)

    def _refused(self, which, nbytes):
        return self.capi.DAU_INVALID_ARGUMENT if nbytes < self.plan.workspace_bytes(which) else None

    def dau_conv_forward(self, h, st, x, w, m1, m2, sg, y, ws, nbytes):
        if self._refused(1, nbytes):
            return self.capi.DAU_INVALID_ARGUMENT
        self._zero(y, self.ybytes)
        self._zero(ws, 16)
        if self.damage:
            name, off, n = self.damage
            ends = dict(y=y.value + self.ybytes, x=x.value + self.xbytes, workspace=ws.value + nbytes, w=w.value + self.pbytes)
            ctypes.memset(ends[name] + off, 0x11, n)
        return self.capi.DAU_OK

    def dau_conv_backward(self, h, st, x, dy, w, m1, m2, sg, dx, dw, d1, d2, ds, ws, nbytes, mask):
        if self._refused(2, nbytes):
            return self.capi.DAU_INVALID_ARGUMENT
        self._zero(dx, self.xbytes)
        for p in (dw, d1, d2, ds):
            self._zero(p, self.pbytes)
        self._zero(ws, 16)
        return self.capi.DAU_OK

    def dau_conv_backward_param_sums(self, h, st, x, dy, m1, m2, sg, sums, ws, nbytes):
        if self._refused(2, nbytes):
            return self.capi.DAU_INVALID_ARGUMENT
        self._zero(sums, 4 * self.pbytes)
        self._zero(ws, 16)
        return self.capi.DAU_OK

    def dau_conv_finalize_param_grads(self, h, st, sums, w, dw, d1, d2, ds, mask):
        for p in (dw, d1, d2, ds):
            self._zero(p, self.pbytes)
        return self.capi.DAU_OK

    def dau_conv_check_status(self, h, st, ws, mx):
        mx._obj.value = 2.5
        return self.capi.DAU_OK


@pytest.fixture
def stand_in(monkeypatch):
    import types
    from dau_conv import _capi
    monkeypatch.setattr(aa, "DEVICE", "cpu")

    def make(io):
        plan = _capi.Plan(3, 5, 9, 3, 13, 21, flags=_capi.FLAG_USE_INTERPOLATION | {"f32": 0, "bf16": _capi.FLAG_IO_BF16, "f16": _capi.FLAG_IO_F16}[io])
        capi = types.SimpleNamespace(**{k: getattr(_capi, k) for k in dir(_capi) if k.isupper()})
        capi.lib = _StandIn(_capi, plan, aa.ESIZE[io])
        rs = np.random.RandomState(1)
        inputs = dict(x=rs.rand(3, 5, 13, 21), dy=rs.randn(3, 9, 13, 21))
        inputs.update({n: rs.randn(1, 5, 3, 9) for n in ("w", "mu1", "mu2", "sigma")})
        return capi, plan, {k: v.astype(np.float32) for k, v in inputs.items()}
    return make


@pytest.mark.parametrize("io", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("skew", [0, 1])
def test_harness_reports_a_well_behaved_call_as_clean(stand_in, io, skew):
    capi, plan, inputs = stand_in(io)
    f = aa.forward(capi, plan, inputs, io, skew, 0xFF)
    assert f.rc == 0 and f.status_rc == 0 and f.max_abs_mu == np.float32(2.5)
    f.assert_clean()
    assert sorted(f.outputs) == ["y"] and f.outputs["y"].shape == (3, 9, 13, 21) and not f.values["y"].any()
    assert sorted(f.untouched) == ["dmu1", "dmu2", "dsigma", "dw", "dx"] and all(f.untouched.values())
    b = aa.backward(capi, plan, inputs, io, skew, 0x7B, need_mask=capi.NEED_DX | capi.NEED_DMU1)
    b.assert_clean()
    assert sorted(b.outputs) == ["dmu1", "dx"] and sorted(b.untouched) == ["dmu2", "dsigma", "dw", "y"]
    assert b.outputs["dx"].dtype == (np.float32 if io == "f32" else np.uint16) and b.outputs["dmu1"].dtype == np.float32
    p = aa.param_sums_finalize(capi, plan, inputs, io, skew, 0x00)
    p.assert_clean()
    assert sorted(p.outputs) == ["dmu1", "dmu2", "dsigma", "dw", "sums"] and p.outputs["sums"].shape == (4, 5, 3, 9)
    for call in (aa.forward, aa.backward, aa.param_sums_finalize):
        r = call(capi, plan, inputs, io, skew, 0x7B, declared_short=1)
        assert r.rc == capi.DAU_INVALID_ARGUMENT and r.status_rc is None and not r.outputs
        assert r.untouched["workspace"] and all(r.untouched.values())


@pytest.mark.parametrize("damage, what, count", [
    (("y", 0, 3), "before_dx", 3),                  # three bytes past the end of y
    (("workspace", 0, 1), "after_workspace", 1),    # one byte past a workspace of exactly workspace_bytes
    (("workspace", -1, 2), "after_workspace", 1),   # the workspace's last byte and the one behind it
    (("x", 5, 1), "before_dy", 1),                  # a lone byte inside a band
    (("x", -4, 4), "x", 0),                         # an input overwritten
    (("w", -4, 4), "w", 0),
])
def test_harness_reports_every_kind_of_damage(stand_in, damage, what, count):
    capi, plan, inputs = stand_in("f16")
    capi.lib.damage = damage
    f = aa.forward(capi, plan, inputs, "f16", 1, 0xFF)
    with pytest.raises(AssertionError):
        f.assert_clean()
    if what in ("x", "w"):
        assert f.inputs_changed == [what] and not f.canaries
    else:
        assert f.canaries == [(what, count, max(damage[1], 0))] and not f.inputs_changed


def test_harness_reports_a_write_to_an_output_that_was_not_requested(stand_in):
    capi, plan, inputs = stand_in("f32")
    capi.lib.damage = ("y", 1 << 20, 1)          # over the band behind y: into dx (skew 0: dx begins right there), which forward must not touch
    f = aa.forward(capi, plan, inputs, "f32", 0, 0x7B)
    assert f.untouched["dx"] is False or f.canaries       # (the band is at least, not exactly, 1 MiB)
    with pytest.raises(AssertionError):
        f.assert_clean()


def _same_report(a, b):
    assert (a.rc, a.status_rc, a.max_abs_mu) == (b.rc, b.status_rc, b.max_abs_mu)
    assert a.canaries == b.canaries and a.inputs_changed == b.inputs_changed and a.untouched == b.untouched
    assert sorted(a.outputs) == sorted(b.outputs) and sorted(a.values) == sorted(b.values)
    for n in a.outputs:
        assert a.outputs[n].dtype == b.outputs[n].dtype and a.outputs[n].shape == b.outputs[n].shape
        assert np.array_equal(aa.as_bits(a.outputs[n]), aa.as_bits(b.outputs[n])), n
        assert np.array_equal(aa.as_bits(a.values[n]), aa.as_bits(b.values[n])), n


@pytest.mark.parametrize("io", ["f32", "f16"])
def test_enqueue_then_finish_is_the_combined_call(stand_in, io):
    """The two halves the concurrency tests use -- enqueue_*(), later Arena.finish() -- leave exactly the Report of forward() /
    backward() / param_sums_finalize(): accepted and refused calls, a prebuilt arena, and a call whose damage the report names."""
    capi, plan, inputs = stand_in(io)
    pairs = ((aa.forward, aa.enqueue_forward, {}), (aa.backward, aa.enqueue_backward, dict(need_mask=capi.NEED_DX | capi.NEED_DW)),
             (aa.backward, aa.enqueue_backward, {}), (aa.param_sums_finalize, aa.enqueue_param_sums_finalize, {}))
    for short in (0, 1):
        for whole, half, kw in pairs:
            want = whole(capi, plan, inputs, io, 1, 0x7B, declared_short=short, **kw)
            a, rc, requested = half(capi, plan, inputs, io, 1, 0x7B, declared_short=short, **kw)
            assert isinstance(a, aa.Arena) and rc == want.rc and sorted(requested) == sorted(want.outputs)
            _same_report(a.finish(rc, requested), want)
    # several calls enqueued before the first is finished, one of them into an arena built ahead of the call
    ahead = aa.Arena(capi, plan, inputs, io, capi.PASS_BACKWARD, 1, 0xFF)
    pending = [aa.enqueue_forward(capi, plan, inputs, io, 1, 0xFF), aa.enqueue_backward(capi, plan, inputs, io, 1, 0xFF, arena=ahead),
               aa.enqueue_param_sums_finalize(capi, plan, inputs, io, 1, 0xFF)]
    assert pending[1][0] is ahead
    for (a, rc, requested), whole in zip(pending, (aa.forward, aa.backward, aa.param_sums_finalize)):
        _same_report(a.finish(rc, requested), whole(capi, plan, inputs, io, 1, 0xFF))
    capi.lib.damage = ("y", 0, 3)
    a, rc, requested = aa.enqueue_forward(capi, plan, inputs, io, 1, 0xFF)
    rep = a.finish(rc, requested)
    _same_report(rep, aa.forward(capi, plan, inputs, io, 1, 0xFF))
    assert rep.canaries == [("before_dx", 3, 0)]
