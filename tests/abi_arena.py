"""A harness that owns every byte the C ABI may touch (helper module of test_abi_arena.py and test_gpu_memory_contract.py).

Every call gets ONE torch.uint8 allocation, the arena.  The buffers of the call are carved out of it in a fixed order -- x, dy, w,
mu1, mu2, sigma, y, dx, dw, dmu1, dmu2, dsigma, sums, workspace -- and every byte of the arena that belongs to no buffer is canary:
at least 1 MiB in front of and behind each buffer, filled with 0xFF (a NaN as fp32, as bfloat16 and as binary16).  An overrun of a
few rows or tiles therefore lands in a canary band of the same allocation -- it changes a canary, it cannot fault -- and a read
out of bounds that reaches an output shows up as a NaN.  The workspace is carved at exactly dau_conv_workspace_bytes(plan, pass),
256-byte aligned (what hipMalloc gives a C host), and that exact number is what the call is told; workspace and outputs are
pre-filled with a poison byte of the caller's choice.  `skew` moves the bases of the activation buffers (x, dy, y, dx) that many
ELEMENTS off their 256-byte alignment; parameters stay aligned.

The harness calls the library through ctypes itself (dau_conv._capi.lib), on torch's current stream; dau_conv._capi.Plan only
creates the plan.

forward(), backward() and param_sums_finalize() run one call to its end.  Each is also there in two halves for the tests that keep
several calls of one plan in flight (test_gpu_concurrency.py): enqueue_forward() / enqueue_backward() /
enqueue_param_sums_finalize() build the arena on torch's current stream -- which is what makes an arena belong to a stream and,
inside a threading.Thread, to that thread -- call the library and return (arena, rc, requested) without waiting; Arena.finish(rc,
requested) waits for the device and reads everything back.
"""
import ctypes
from collections import OrderedDict, namedtuple

import numpy as np

BAND = 1 << 20            # least canary bytes in front of and behind every buffer
ALIGN = 256               # hipMalloc's alignment: the workspace base, and every other base before its skew
CANARY = 0xFF
FILLS = (0x00, 0xFF, 0x7B)   # 0x7B7B7B7B ~ 1.3e36 as fp32, 0x7B7B = 63328 as f16, large and finite as bf16
DEVICE = "cuda"           # test_abi_arena.py sets "cpu": the harness's own bookkeeping, checked in host memory against a stand-in library

ORDER = ("x", "dy", "w", "mu1", "mu2", "sigma", "y", "dx", "dw", "dmu1", "dmu2", "dsigma", "sums", "workspace")
ACTIVATIONS = ("x", "dy", "y", "dx")
INPUTS = ("x", "dy", "w", "mu1", "mu2", "sigma")
OUTPUTS = ("y", "dx", "dw", "dmu1", "dmu2", "dsigma", "sums")
GRADS = ("dw", "dmu1", "dmu2", "dsigma")
ESIZE = {"f32": 4, "bf16": 2, "f16": 2}

Region = namedtuple("Region", "name offset size")
Layout = namedtuple("Layout", "total regions bands")      # regions: OrderedDict name -> Region; bands: list of Region (canaries)


def layout(sizes, esize, skew=0, band=BAND):
    """Carve an arena whose base is ALIGN-aligned: sizes {name: bytes} (names of ORDER; a missing or zero-sized buffer gets no
    region) -> Layout.  A pure function of its arguments.  Every byte outside the regions is canary; the band in front of a buffer
    ends where the buffer begins, the band behind it begins where the buffer ends."""
    regions, bands = OrderedDict(), []
    pos = 0                                            # end of the previous buffer
    for name in ORDER:
        size = int(sizes.get(name, 0))
        if size <= 0:
            continue
        base = -(-(pos + band) // ALIGN) * ALIGN
        if name in ACTIVATIONS:
            base += skew * esize
        bands.append(Region("before_" + name, pos, base - pos))
        regions[name] = Region(name, base, size)
        pos = base + size
    total = pos + band
    bands.append(Region("after_" + next(reversed(regions)), pos, band))
    return Layout(total, regions, bands)


def to_storage(a, io):
    """float32 array -> the array the kernels read: float32, or the uint16 bit patterns of its bfloat16 / binary16 rounding"""
    a = np.ascontiguousarray(a, np.float32)
    if io == "f32":
        return a
    if io == "f16":
        return a.astype(np.float16).view(np.uint16)
    u = a.view(np.uint32)                              # bfloat16: round to nearest even on the bits (finite inputs)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(bits, io):
    """stored array (to_storage's format) -> the float32 values it holds"""
    if io == "f32":
        return np.asarray(bits, np.float32)
    if io == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def as_bits(a):
    """an unsigned-integer view: NaN-proof equality"""
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


class Report(object):
    """What one call left behind.  rc: the entry point's return code (the second one for sums + finalize); status_rc / max_abs_mu:
    dau_conv_check_status (None when the call was refused); outputs: {name: stored array} of the requested outputs, values: the same
    widened to float32; canaries: [(band, bytes changed, first changed offset in the band)] of the damaged bands; inputs_changed:
    names of inputs that differ from what was uploaded; untouched: {name: bool} for the workspace (refused calls) and every output
    that was NOT requested -- True if it still holds its fill in every byte."""

    def __init__(self):
        self.rc = self.status_rc = self.max_abs_mu = None
        self.outputs, self.values, self.untouched = {}, {}, {}
        self.canaries, self.inputs_changed = [], []

    def assert_clean(self, tag=""):
        assert not self.canaries, "%s: canary bands damaged (band, bytes, first offset): %s" % (tag, self.canaries)
        assert not self.inputs_changed, "%s: inputs changed by the call: %s" % (tag, self.inputs_changed)
        bad = [n for n, ok in self.untouched.items() if not ok]
        assert not bad, "%s: buffers the call had no business with were written: %s" % (tag, bad)


class Arena(object):
    """One call's memory.  inputs: {x, dy, w, mu1, mu2, sigma: float32 arrays} (x, dy are stored in the plan's format)."""

    def __init__(self, capi, plan, inputs, io, which, skew=0, fill=0xFF, with_sums=False):
        import torch
        self.capi, self.plan, self.io, self.fill, self.which = capi, plan, io, fill, which
        self.ws_bytes = plan.workspace_bytes(which)
        self.host = {n: to_storage(inputs[n], io if n in ACTIVATIONS else "f32") for n in INPUTS}
        units = plan.S * plan.G * plan.F
        es = ESIZE[io]
        sizes = {n: self.host[n].nbytes for n in INPUTS}
        sizes.update(y=plan.N * plan.F * plan.H * plan.W * es, dx=plan.N * plan.S * plan.H * plan.W * es,
                     dw=4 * units, dmu1=4 * units, dmu2=4 * units, dsigma=4 * units, workspace=self.ws_bytes)
        if with_sums:
            sizes["sums"] = 16 * units
        self.shapes = dict(y=(plan.N, plan.F, plan.H, plan.W), dx=(plan.N, plan.S, plan.H, plan.W), sums=(4, plan.S, plan.G, plan.F))
        for n in GRADS:
            self.shapes[n] = (1, plan.S, plan.G, plan.F)
        self.lay = layout(sizes, es, skew)
        raw = torch.empty(self.lay.total + ALIGN, dtype=torch.uint8, device=DEVICE)
        lead = -raw.data_ptr() % ALIGN
        self.mem = raw[lead:lead + self.lay.total]
        assert self.mem.data_ptr() % ALIGN == 0
        self.mem.fill_(CANARY)
        for n, r in self.lay.regions.items():
            if n in INPUTS:
                self.mem[r.offset:r.offset + r.size].copy_(torch.from_numpy(self.host[n].view(np.uint8).reshape(-1)))
            else:
                self.mem[r.offset:r.offset + r.size].fill_(fill)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if DEVICE == "cuda" else None

    def ptr(self, name, wanted=True):
        if not wanted:
            return None
        return ctypes.c_void_p(self.mem.data_ptr() + self.lay.regions[name].offset)

    def _bytes(self, name):
        r = self.lay.regions[name]
        return self.mem[r.offset:r.offset + r.size]

    def finish(self, rc, requested, check_status=True):
        """sync, read everything back -> Report"""
        import torch
        rep = Report()
        rep.rc = rc
        if rc == self.capi.DAU_OK and check_status:
            mx = ctypes.c_float()
            rep.status_rc = self.capi.lib.dau_conv_check_status(self.plan._h, self.stream, self.ptr("workspace"), ctypes.byref(mx))
            rep.max_abs_mu = np.float32(mx.value)
        if DEVICE == "cuda":
            torch.cuda.synchronize()
        changed = torch.stack([(self.mem[b.offset:b.offset + b.size] != CANARY).sum() for b in self.lay.bands]).cpu().numpy()
        for b, n in zip(self.lay.bands, changed):
            if n:
                first = int(torch.nonzero(self.mem[b.offset:b.offset + b.size] != CANARY)[0])
                rep.canaries.append((b.name, int(n), first))
        for n in INPUTS:
            if not np.array_equal(self._bytes(n).cpu().numpy(), self.host[n].view(np.uint8).reshape(-1)):
                rep.inputs_changed.append(n)
        for n in OUTPUTS:
            if n not in self.lay.regions:
                continue
            got = self._bytes(n).cpu().numpy()
            if n in requested:
                dt = np.float32 if (n not in ACTIVATIONS or self.io == "f32") else np.uint16
                rep.outputs[n] = got.view(dt).reshape(self.shapes[n]).copy()
                rep.values[n] = widen(rep.outputs[n], self.io if n in ACTIVATIONS else "f32")
            else:
                rep.untouched[n] = bool((got == self.fill).all())
        if rc != self.capi.DAU_OK:
            rep.untouched["workspace"] = bool((self._bytes("workspace") == self.fill).all())
        return rep


def enqueue_forward(capi, plan, inputs, io="f32", skew=0, fill=0xFF, declared_short=0, arena=None):
    """The enqueue half of forward(): an arena on torch's current stream, dau_conv_forward on that stream -> (arena, rc, requested).
    Nothing waits for the call; arena.finish(rc, requested) does, and a test that wants several calls in flight finishes none
    before it has enqueued them all.  arena: one the caller built earlier with the same arguments (building one uploads its inputs,
    which makes the host wait for the stream), so that a burst of calls is enqueued with nothing between them."""
    a = arena or Arena(capi, plan, inputs, io, capi.PASS_FORWARD, skew, fill)
    rc = capi.lib.dau_conv_forward(plan._h, a.stream, a.ptr("x"), a.ptr("w"), a.ptr("mu1"), a.ptr("mu2"), a.ptr("sigma"), a.ptr("y"),
                                   a.ptr("workspace"), a.ws_bytes - declared_short)
    return a, rc, ("y",) if rc == capi.DAU_OK else ()


def forward(capi, plan, inputs, io="f32", skew=0, fill=0xFF, declared_short=0, outlier_status=False):
    """dau_conv_forward in an arena of its own -> Report (declared_short: bytes by which the declared workspace size is reduced;
    outlier_status: also dau_conv_gather_outlier_status on the arena's workspace -> report.outliers = (units, ring_taken))"""
    a, rc, requested = enqueue_forward(capi, plan, inputs, io, skew, fill, declared_short)
    rep = a.finish(rc, requested)
    if outlier_status:
        rep.outliers = _outlier_status(capi, plan, a)
    return rep


def _requested(capi, need_mask):
    bits = (("dx", capi.NEED_DX), ("dw", capi.NEED_DW), ("dmu1", capi.NEED_DMU1), ("dmu2", capi.NEED_DMU2), ("dsigma", capi.NEED_DSIGMA))
    return tuple(n for n, b in bits if need_mask & b)


def enqueue_backward(capi, plan, inputs, io="f32", skew=0, fill=0xFF, need_mask=None, declared_short=0, arena=None):
    """The enqueue half of backward() -> (arena, rc, requested); see enqueue_forward"""
    need_mask = capi.NEED_ALL if need_mask is None else need_mask
    a = arena or Arena(capi, plan, inputs, io, capi.PASS_BACKWARD, skew, fill)
    req = _requested(capi, need_mask)
    rc = capi.lib.dau_conv_backward(plan._h, a.stream, a.ptr("x"), a.ptr("dy"), a.ptr("w"), a.ptr("mu1"), a.ptr("mu2"), a.ptr("sigma"),
                                    *([a.ptr(n, n in req) for n in ("dx",) + GRADS] + [a.ptr("workspace"), a.ws_bytes - declared_short,
                                                                                      int(need_mask)]))
    return a, rc, req if rc == capi.DAU_OK else ()


def backward(capi, plan, inputs, io="f32", skew=0, fill=0xFF, need_mask=None, declared_short=0, outlier_status=False):
    """dau_conv_backward in an arena of its own; a gradient that need_mask does not request is passed as NULL -> Report
    (outlier_status: also dau_conv_gather_outlier_status on the arena's workspace -> report.outliers = (units, ring_taken))"""
    a, rc, requested = enqueue_backward(capi, plan, inputs, io, skew, fill, need_mask, declared_short)
    rep = a.finish(rc, requested)
    if outlier_status:
        rep.outliers = _outlier_status(capi, plan, a)
    return rep


def _outlier_status(capi, plan, arena):
    units, taken = ctypes.c_int32(), ctypes.c_int32()
    rc = capi.lib.dau_conv_gather_outlier_status(plan._h, arena.stream, arena.ptr("workspace"), ctypes.byref(units), ctypes.byref(taken))
    assert rc == capi.DAU_OK
    return units.value, bool(taken.value)


def enqueue_param_sums_finalize(capi, plan, inputs, io="f32", skew=0, fill=0xFF, declared_short=0, arena=None):
    """The enqueue half of param_sums_finalize() -> (arena, rc, requested): rc is the second entry point's, or the first's if that
    refused the call (then nothing is requested); see enqueue_forward"""
    a = arena or Arena(capi, plan, inputs, io, capi.PASS_BACKWARD, skew, fill, with_sums=True)
    rc = capi.lib.dau_conv_backward_param_sums(plan._h, a.stream, a.ptr("x"), a.ptr("dy"), a.ptr("mu1"), a.ptr("mu2"), a.ptr("sigma"),
                                               a.ptr("sums"), a.ptr("workspace"), a.ws_bytes - declared_short)
    if rc != capi.DAU_OK:
        return a, rc, ()
    mask = capi.NEED_DW | capi.NEED_DMU1 | capi.NEED_DMU2 | capi.NEED_DSIGMA
    rc = capi.lib.dau_conv_finalize_param_grads(plan._h, a.stream, a.ptr("sums"), a.ptr("w"), a.ptr("dw"), a.ptr("dmu1"), a.ptr("dmu2"),
                                                a.ptr("dsigma"), mask)
    return a, rc, GRADS + ("sums",)


def param_sums_finalize(capi, plan, inputs, io="f32", skew=0, fill=0xFF, declared_short=0):
    """dau_conv_backward_param_sums into a poisoned `sums` buffer, then dau_conv_finalize_param_grads of the four kinds -> Report"""
    a, rc, requested = enqueue_param_sums_finalize(capi, plan, inputs, io, skew, fill, declared_short)
    return a.finish(rc, requested)
