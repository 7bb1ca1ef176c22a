"""GPU: the concurrency contract of the C ABI (include/dau_conv.h): "a plan's configuration is immutable after creation, so
concurrent calls on different streams with different workspaces are safe", "a plan may be used on any device (the kernels' launch
attributes are set once per device, on the first call there, behind a lock)", dau_conv_last_error is "thread-local", the status
block belongs to the workspace and the pinned mirror to the plan.  Every other GPU test is one host thread with one call in flight;
here one plan has up to four calls in flight, on four streams and from four host threads.

Plan families (each: one plan per test, asserted to hold the paths it is here for):
  split-k17           USE_INTERPOLATION | DENSE_SPLIT_F16, max_kernel_size 17, float32, N=2 S=6 F=24 G=4 28 x 28
  exact-k33-f16-nhwc  USE_INTERPOLATION | NO_DENSE_SPLIT | IO_F16 | IO_NHWC, max_kernel_size 33, the ragged shape of
                      test_gpu_memory_contract.py (N=3 S=5 F=9 G=3 13 x 21)
  line                USE_INTERPOLATION | SINGLE_DIM_KERNEL | DENSE_SPLIT_F16 | DENSE_SPLIT_LINE | SPLIT_DOT_LINE, max_kernel_size 17,
                      N=9 S=7 F=5 G=2 9 x 6: the case of test_gpu_line_dot.py with the fewest multiply-adds
Lanes: four input sets per family whose calls need DIFFERENT kernels of the one plan, so that the offset-bucket hint every call
leaves in the plan's pinned mirror is wrong for most of the calls that read it: lanes 0-2 differ in their offsets (see FAMILIES),
lane 3 has lane 0's parameters and another x and dy.

Yardstick: every (family, lane) runs forward + backward ALONE -- a plan that has made no other call, the combined arena calls of
abi_arena.py, synchronised -- and that run is compared with oracle.dau_oracle at the project's existing bars (util.assert_parity
defaults for float32; rel 2e-3 / floor 1e-3 for y and dx in f16 storage, test_gpu_f16.py).  Everything concurrent is then compared
BIT FOR BIT with that serial run: no tolerance of its own anywhere in this module.

What this module found when it was written: the parameter gradients of the exact-k33 family's lanes differed from their serial
runs in most bits (inside the parity bar) whenever another lane's max|mu| was the hint they read -- the tiled gather-dot's sums come
in another order in every bucket set, and the hint chose the set.  That pass now takes no hint (pick_candidates, dau_conv_api.hip).
And test_python_plan_queries_follow_the_calling_thread's first thread was told about the second thread's call: dau_conv._capi.Plan
kept "the last call" in one attribute per plan; it now keeps it per (device, stream) and thread.

Each test is one pass: nothing is repeated until it races, and nothing here is meant to fault -- NaN and out-of-range offsets and
short or null arguments are inputs the library handles or refuses, all used by other tests already.  A thread that has not come back
after JOIN_SECONDS fails its test, which then makes no further GPU call."""
import ctypes
import json
import os
import threading

import numpy as np
import pytest
import torch

import abi_arena as aa
from oracle import dau_oracle as orc
from util import assert_parity, make_inputs

pytestmark = pytest.mark.gpu

PARAMS = aa.GRADS
ROUNDS, NLANES, JOIN_SECONDS = 3, 4, 120
SKEW, FILL = 1, 0xFF
I, SD, SPLIT, NO_SPLIT, F16, NHWC, LINE, DOT_LINE = 1 << 0, 1 << 2, 1 << 9, 1 << 10, 1 << 11, 1 << 13, 1 << 15, 1 << 16


class Family(object):
    """name; shape (N, S, F, G, H, W); max_kernel_size; flags; storage; m: the offset range of lanes 0-2; holds(info): the plan
    holds the paths the family is here for"""

    def __init__(self, name, shape, k, flags, m, holds, io="f32", seed=0):
        self.name, self.shape, self.k, self.flags, self.m, self.holds, self.io, self.seed = name, shape, k, flags, m, holds, io, seed
        self.nhwc, self.single_dim = bool(flags & NHWC), bool(flags & SD)

    def plan(self, k=None):
        from dau_conv import _capi
        plan = _capi.Plan(*self.shape, max_kernel_size=k or self.k, flags=self.flags, sigma_hint=0.5)
        if k is None:
            assert self.holds(plan.info), "%s: the plan lacks the paths this family tests: %r" % (self.name, plan.info)
        return plan


FAMILIES = {f.name: f for f in (
    # lanes: within +-2 (radius-2 member), within +-3.9 with a unit at 3.99 (radius 4), within +-7.5 (the exact kernels of bucket 8)
    Family("split-k17", (2, 6, 24, 4, 28, 28), 17, I | SPLIT, (2.0, 3.9, 7.5), seed=1700,
           holds=lambda i: i["bucket_sets"] >= 2 and i["gather_dense_split"] & 0b11100 == 0b11100),
    # lanes: the exact kernels of buckets 4, 8 and 16
    Family("exact-k33-f16-nhwc", (3, 5, 9, 3, 13, 21), 33, I | NO_SPLIT | F16 | NHWC, (3.0, 7.5, 15.5), io="f16", seed=3300,
           holds=lambda i: i["bucket_sets"] >= 2 and i["gather_dense_split"] == 0),
    # lanes: on the line within +-3.9 (line members of radius 4), on the line within +-7.5 (radius 8), three units off the line
    Family("line", (9, 7, 5, 2, 9, 6), 17, I | SD | SPLIT | LINE | DOT_LINE, (3.9, 7.5, 3.9), seed=1900,
           holds=lambda i: i["gather_dense_split"] & (3 << 6) == 3 << 6 and i["gather_dense_split"] & (3 << 8) == 3 << 8),
)}
NAMES = sorted(FAMILIES)
OFF_LINE = ((5, 0.25), (17, -1.5), (40, 2.75))        # (flat index, mu2) of the line family's lane 2

_INPUTS, _ORACLE, _YARD = {}, {}, {}


def _inputs(fam, lane):
    """{x, dy, w, mu1, mu2, sigma} of a lane, in NCHW float32 (computed once, never written: a test that changes an offset copies the array)"""
    key = (fam.name, lane)
    if key not in _INPUTS:
        base = 0 if lane == 3 else lane
        x, dy, w, mu1, mu2 = make_inputs(fam.seed + base, *fam.shape, fam.k, fam.m[base])
        if lane == 3:
            x, dy = make_inputs(fam.seed + 3, *fam.shape, fam.k, fam.m[base])[:2]
        if fam.name == "split-k17" and base == 1:
            mu1.flat[0] = 3.99
        if fam.single_dim:
            mu2[:] = 0
            if base == 2:
                for idx, v in OFF_LINE:
                    mu2.flat[idx] = v
        mx = max(np.abs(mu1).max(), np.abs(mu2).max())
        lo, hi = {"split-k17": ((0, 2), (3, 4), (4, 8)), "exact-k33-f16-nhwc": ((0, 4), (4, 8), (8, 16)),
                  "line": ((0, 4), (4, 8), (0, 4))}[fam.name][base]
        assert lo < mx <= hi, "%s lane %d: max|mu| %r was meant to lie in (%d, %d]" % (fam.name, lane, mx, lo, hi)
        S, G, F = w.shape[1:]
        _INPUTS[key] = dict(x=x, dy=dy, w=w, mu1=mu1, mu2=mu2, sigma=np.full((1, S, G, F), 0.5, np.float32))
    return _INPUTS[key]


def _arena_inputs(fam, inputs):
    """what the arena uploads: an NHWC plan gets [N][H][W][C] arrays"""
    if not fam.nhwc:
        return inputs
    return dict(inputs, x=np.ascontiguousarray(inputs["x"].transpose(0, 2, 3, 1)), dy=np.ascontiguousarray(inputs["dy"].transpose(0, 2, 3, 1)))


def _nchw(fam, name, v):
    """an activation of a report (shaped NCHW over the plan's memory order) as the NCHW array it stands for"""
    if not fam.nhwc or name not in aa.ACTIVATIONS:
        return v
    n, c, h, w = v.shape
    return v.reshape(n, h, w, c).transpose(0, 3, 1, 2)


def _oracle(fam, lane):
    key = (fam.name, lane)
    if key not in _ORACLE:
        d = _inputs(fam, lane)
        xr, dyr = (aa.widen(aa.to_storage(d[n], fam.io), fam.io) for n in ("x", "dy"))      # what the kernels read
        want = dict(orc.backward(xr, dyr, d["w"], d["mu1"], d["mu2"], 0.5, single_dim_kernel=fam.single_dim))
        want["y"] = orc.forward(xr, d["w"], d["mu1"], d["mu2"], 0.5, single_dim_kernel=fam.single_dim)
        _ORACLE[key] = want
    return _ORACLE[key]


def _max_abs_mu(d):
    return np.float32(max(np.abs(d["mu1"]).max(), np.abs(d["mu2"]).max()))


def _check_report(rep, d, tag):
    from dau_conv import _capi
    assert rep.rc == _capi.DAU_OK, "%s: rc %d: %s" % (tag, rep.rc, _capi.lib.dau_conv_last_error())
    rep.assert_clean(tag)
    assert rep.status_rc == _capi.DAU_OK, "%s: check_status %d" % (tag, rep.status_rc)
    # the status block belongs to the WORKSPACE of the call, not to the plan: this lane's maximum, whatever ran beside it
    assert rep.max_abs_mu == _max_abs_mu(d), "%s: max|mu| %r, numpy says %r for this lane" % (tag, rep.max_abs_mu, _max_abs_mu(d))


def _yardstick(fam, lane):
    """{output: bits} of the lane's forward + backward run alone on a fresh plan, compared with the oracle (once per lane)"""
    from dau_conv import _capi
    key = (fam.name, lane)
    if key not in _YARD:
        d, plan = _inputs(fam, lane), fam.plan()
        tag = "%s lane %d alone" % (fam.name, lane)
        f = aa.forward(_capi, plan, _arena_inputs(fam, d), fam.io, SKEW, FILL)
        _check_report(f, d, tag + " forward")
        b = aa.backward(_capi, plan, _arena_inputs(fam, d), fam.io, SKEW, FILL)
        _check_report(b, d, tag + " backward")
        want = _oracle(fam, lane)
        io_bar = dict(rel=2e-3, floor=1e-3) if fam.io == "f16" else {}
        values = dict(f.values, **b.values)
        for n in ("y", "dx") + PARAMS:
            assert_parity(_nchw(fam, n, values[n]), want[n], "%s %s" % (tag, n), **(io_bar if n in aa.ACTIVATIONS else {}))
        _YARD[key] = {n: aa.as_bits(v) for n, v in dict(f.outputs, **b.outputs).items()}
    return _YARD[key]


def _differences(rep, yard, tag, names=None):
    """-> one line per output of the report that is not the lane's serial bits"""
    out = []
    for n in sorted(names or rep.outputs):
        got = aa.as_bits(rep.outputs[n])
        differ = int((got != yard[n]).sum())
        if differ:
            out.append("%s: %s differs from the lane's serial run in %d of %d values (first at flat index %d)" % (
                tag, n, differ, got.size, int(np.flatnonzero(got != yard[n])[0])))
    return out


def _assert_yardstick(rep, yard, tag, names=None):
    bad = _differences(rep, yard, tag, names)
    assert not bad, "\n".join(bad)


def _finish_and_check(fam, pending, yards):
    """pending: [(lane, round, what, arena, rc, requested)] -- read back only now that every call of the test has been enqueued.
    Return codes, canaries and statuses are asserted call by call; the bit differences of all calls are reported together, so
    that a failure shows which lanes, rounds and tensors it touches."""
    bad = []
    for lane, rnd, what, arena, rc, requested in pending:
        tag = "%s lane %d round %d %s" % (fam.name, lane, rnd, what)
        rep = arena.finish(rc, requested)
        _check_report(rep, _inputs(fam, lane), tag)
        bad += _differences(rep, yards[lane], tag, [n for n in rep.outputs if n != "sums"])
    assert not bad, "%d outputs differ from their lane's serial run:\n%s" % (len(bad), "\n".join(bad))


def _record_overlap(record):
    """one line per family into $DAU_TEST_RECORD_DIR/concurrency_overlap.jsonl where that variable names a directory (the file is
    kept under profiles/); the figure is printed either way"""
    out = os.environ.get("DAU_TEST_RECORD_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "concurrency_overlap.jsonl"), "a") as fh:
            fh.write(json.dumps(record) + "\n")


_ARENA_KW = {"forward": "PASS_FORWARD", "backward": "PASS_BACKWARD"}
_ENQUEUE = {"forward": aa.enqueue_forward, "backward": aa.enqueue_backward}


# ---- 1. one host thread, four streams ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_streams_interleaved(name):
    """Three rounds of forward on every lane's stream, then backward on every lane's stream: 24 calls of one plan, each in a fresh
    arena (fill 0xFF, skew 1), and no synchronisation of any kind between the first call and the last.  The arenas are built and
    uploaded before the first call, so that the host enqueues the 24 calls back to back.  The number of pairs of calls on different
    streams whose [start, end] event intervals overlapped is printed and recorded, not asserted: overlap cannot be forced."""
    from dau_conv import _capi
    fam = FAMILIES[name]
    yards = [_yardstick(fam, lane) for lane in range(NLANES)]
    plan = fam.plan()
    streams = [torch.cuda.Stream() for _ in range(NLANES)]
    order = [(rnd, what, lane) for rnd in range(ROUNDS) for what in ("forward", "backward") for lane in range(NLANES)]
    arenas = {}
    for rnd, what, lane in order:
        with torch.cuda.stream(streams[lane]):
            arenas[rnd, what, lane] = aa.Arena(_capi, plan, _arena_inputs(fam, _inputs(fam, lane)), fam.io, getattr(_capi, _ARENA_KW[what]),
                                               SKEW, FILL)
    torch.cuda.synchronize()                                 # every upload has landed; from here on nothing waits
    start = torch.cuda.Event(enable_timing=True)
    start.record()
    for s in streams:
        s.wait_event(start)
    pending, events = [], []
    for rnd, what, lane in order:
        with torch.cuda.stream(streams[lane]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            a, rc, requested = _ENQUEUE[what](_capi, plan, None, fam.io, SKEW, FILL, arena=arenas[rnd, what, lane])
            e1.record()
        pending.append((lane, rnd, what, a, rc, requested))
        events.append((lane, e0, e1))
    torch.cuda.synchronize()
    spans = [(lane, start.elapsed_time(e0), start.elapsed_time(e1)) for lane, e0, e1 in events]
    pairs = sum(1 for i, (la, a0, a1) in enumerate(spans) for lb, b0, b1 in spans[i + 1:] if la != lb and a0 < b1 and b0 < a1)
    record = dict(test="test_streams_interleaved", family=name, calls=len(spans), overlapping_pairs_on_different_streams=pairs,
                  pairs_on_different_streams=sum(1 for i, a in enumerate(spans) for b in spans[i + 1:] if a[0] != b[0]),
                  first_start_ms=round(min(s[1] for s in spans), 3), last_end_ms=round(max(s[2] for s in spans), 3),
                  summed_call_ms=round(sum(s[2] - s[1] for s in spans), 3))
    print("overlap", json.dumps(record))
    _record_overlap(record)
    _finish_and_check(fam, pending, yards)


# ---- 1b. the same property without a second stream: whatever hint a call reads, it gives its serial bits ------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_serial_calls_do_not_depend_on_the_hint(name):
    """What the interleaved calls rely on, made deterministic: one stream, every call synchronised.  Each lane's backward as the
    FIRST call of a fresh plan (no hint at all), then the lanes' forward + backward one after the other on one plan, in an order in
    which every call reads the hint of a lane that needs other kernels (larger, smaller and equal offsets before it)."""
    from dau_conv import _capi
    fam = FAMILIES[name]
    yards = [_yardstick(fam, lane) for lane in range(NLANES)]
    bad = []
    for lane in range(NLANES):
        d, tag = _inputs(fam, lane), "%s lane %d, backward as a fresh plan's first call" % (fam.name, lane)
        rep = aa.backward(_capi, fam.plan(), _arena_inputs(fam, d), fam.io, SKEW, FILL)
        _check_report(rep, d, tag)
        bad += _differences(rep, yards[lane], tag)
    plan = fam.plan()
    for before, lane in zip((None, 2, 0, 1, 3, 2, 1), (2, 0, 1, 3, 2, 1, 0)):
        d = _inputs(fam, lane)
        for what, call in (("forward", aa.forward), ("backward", aa.backward)):
            tag = "%s lane %d %s after lane %s" % (fam.name, lane, what, before)
            rep = call(_capi, plan, _arena_inputs(fam, d), fam.io, SKEW, FILL)
            _check_report(rep, d, tag)
            bad += _differences(rep, yards[lane], tag)
    assert not bad, "%d outputs differ from their lane's serial run:\n%s" % (len(bad), "\n".join(bad))


# ---- 2. four host threads, the plan's first call under contention --------------------------------------------------------------------
def _join(threads, failures):
    for th in threads:
        th.join(JOIN_SECONDS)
    if any(th.is_alive() for th in threads):
        pytest.fail("a thread has not come back after %d s; no further GPU call is made" % JOIN_SECONDS, pytrace=False)
    for e in failures:
        if e is not None:
            raise e


@pytest.mark.parametrize("name", NAMES)
def test_first_call_of_a_plan_from_four_threads(name):
    """A fresh plan; four threads, each with a stream and a lane of its own, make the plan's FIRST call at once (the launch attributes
    behind the plan's lock), then three rounds of forward + backward; the main thread reads everything back."""
    from dau_conv import _capi
    fam = FAMILIES[name]
    yards = [_yardstick(fam, lane) for lane in range(NLANES)]
    plan = fam.plan()
    streams = [torch.cuda.Stream() for _ in range(NLANES)]
    torch.cuda.synchronize()
    barrier = threading.Barrier(NLANES)
    results, failures = [None] * NLANES, [None] * NLANES

    def work(lane):
        try:
            d, mine = _arena_inputs(fam, _inputs(fam, lane)), []
            with torch.cuda.stream(streams[lane]):
                first = aa.Arena(_capi, plan, d, fam.io, _capi.PASS_FORWARD, SKEW, FILL)     # built ahead: after the barrier, the call itself
                barrier.wait(JOIN_SECONDS)
                for rnd in range(ROUNDS):
                    mine.append((lane, rnd, "forward") + aa.enqueue_forward(_capi, plan, d, fam.io, SKEW, FILL, arena=first if rnd == 0 else None))
                    mine.append((lane, rnd, "backward") + aa.enqueue_backward(_capi, plan, d, fam.io, SKEW, FILL))
                streams[lane].synchronize()
            results[lane] = mine
        except BaseException as e:                            # noqa: B902 (kept for the main thread, which raises it)
            failures[lane] = e

    threads = [threading.Thread(target=work, args=(lane,), daemon=True) for lane in range(NLANES)]
    for th in threads:
        th.start()
    _join(threads, failures)
    _finish_and_check(fam, [c for mine in results for c in mine], yards)


# ---- 3. the two-step parameter gradients beside other calls --------------------------------------------------------------------------
def test_param_sums_and_finalize_beside_other_calls():
    """Lane 0: dau_conv_backward_param_sums + dau_conv_finalize_param_grads on one stream, three times, alternating with
    dau_conv_backward of lanes 1-3 on three other streams: the finalised gradients are the bits of the lane's serial dau_conv_backward."""
    from dau_conv import _capi
    fam = FAMILIES["split-k17"]
    yards = [_yardstick(fam, lane) for lane in range(NLANES)]
    plan = fam.plan()
    streams = [torch.cuda.Stream() for _ in range(NLANES)]
    order = [lane for other in (1, 2, 3) for lane in (other, 0)]
    arenas = []
    for lane in order:
        with torch.cuda.stream(streams[lane]):
            arenas.append(aa.Arena(_capi, plan, _inputs(fam, lane), fam.io, _capi.PASS_BACKWARD, SKEW, FILL, with_sums=lane == 0))
    torch.cuda.synchronize()
    pending = []
    for i, (lane, arena) in enumerate(zip(order, arenas)):
        with torch.cuda.stream(streams[lane]):
            enqueue = aa.enqueue_param_sums_finalize if lane == 0 else aa.enqueue_backward
            pending.append((lane, i // 2, "sums + finalize" if lane == 0 else "backward") + enqueue(_capi, plan, None, fam.io, SKEW, FILL, arena=arena))
    assert sorted(pending[1][5]) == sorted(PARAMS + ("sums",))
    _finish_and_check(fam, pending, yards)


# ---- 4. the status block belongs to the workspace, the sticky record to the plan -----------------------------------------------------
def _last_status(plan):
    from dau_conv import _capi
    mx, valid = ctypes.c_float(), ctypes.c_int32()
    rc = _capi.lib.dau_conv_last_status(plan._h, ctypes.byref(mx), ctypes.byref(valid))
    return rc, _capi.lib.dau_conv_last_error() if rc else b""


def _check_status(plan, arena):
    from dau_conv import _capi
    mx = ctypes.c_float()
    rc = _capi.lib.dau_conv_check_status(plan._h, arena.stream, arena.ptr("workspace"), ctypes.byref(mx))
    return rc, np.float32(mx.value), _capi.lib.dau_conv_last_error() if rc else b""


@pytest.mark.parametrize("bad", ["nan", "out-of-range"])
def test_status_belongs_to_the_workspace(bad):
    """Lane A has a bad offset (a NaN, which the kernels read as 0; or 6.0 under max_kernel_size 9, which they clamp), lane B is clean;
    A then B are enqueued on two streams without a sync.  Asked for B's workspace, dau_conv_check_status answers DAU_OK with B's
    maximum, and A's error stays in the plan's sticky record for dau_conv_last_status, once.  (dau_conv_last_status reads what
    COMPLETED calls left: stream A is waited for before it is asked -- after the check of B, which is the one that must not depend on
    it.)  The mirror image in a fresh plan: asked for A's workspace, dau_conv_check_status reports the error, and with that the
    plan's record of it is gone."""
    from dau_conv import _capi
    fam = FAMILIES["split-k17"]
    k, error, word, value = (17, _capi.DAU_FAILED_PRECONDITION, b"NaN", np.nan) if bad == "nan" else (9, _capi.DAU_INVALID_ARGUMENT, b"larger than", 6.0)
    if bad == "nan":
        da, db = dict(_inputs(fam, 0)), _inputs(fam, 1)
    else:                                                    # max_kernel_size 9: offsets within +-2 and within +-3.9
        mk = lambda seed, m: dict(zip(("x", "dy", "w", "mu1", "mu2"), make_inputs(seed, *fam.shape, 9, m)), sigma=_inputs(fam, 0)["sigma"])
        da, db = mk(901, 2.0), mk(902, 3.9)
    da["mu1"] = da["mu1"].copy()
    da["mu1"].flat[0] = value
    want_b = _max_abs_mu(db)
    seen_y = []
    for first in ("B", "A"):
        plan = fam.plan(k)
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(sa):
            a = aa.Arena(_capi, plan, da, fam.io, _capi.PASS_FORWARD, SKEW, FILL)
        with torch.cuda.stream(sb):
            b = aa.Arena(_capi, plan, db, fam.io, _capi.PASS_FORWARD, SKEW, FILL)
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            _, rca, reqa = aa.enqueue_forward(_capi, plan, None, fam.io, SKEW, FILL, arena=a)
        with torch.cuda.stream(sb):
            _, rcb, reqb = aa.enqueue_forward(_capi, plan, None, fam.io, SKEW, FILL, arena=b)
        assert rca == rcb == _capi.DAU_OK
        if first == "B":
            rc, mx, _ = _check_status(plan, b)
            assert rc == _capi.DAU_OK and mx == want_b, (rc, mx, want_b)
            sa.synchronize()
            rc, msg = _last_status(plan)
            assert rc == error and word in msg, (rc, msg)    # A's record survived B's clean report
            assert _last_status(plan)[0] == _capi.DAU_OK     # reported once
        else:
            rc, mx, msg = _check_status(plan, a)
            assert rc == error and word in msg, (rc, msg)
            if bad == "out-of-range":
                assert mx == np.float32(6.0)
            sb.synchronize()
            assert _last_status(plan)[0] == _capi.DAU_OK     # the report of A's workspace took A's record with it
            rc, mx, _ = _check_status(plan, b)
            assert rc == _capi.DAU_OK and mx == want_b, (rc, mx, want_b)
        ra, rb = a.finish(rca, reqa), b.finish(rcb, reqb)
        for rep, tag in ((ra, "A"), (rb, "B")):
            rep.assert_clean("%s, %s asked first: lane %s" % (bad, first, tag))
            assert np.isfinite(rep.values["y"]).all()
        assert ra.status_rc == error and rb.status_rc == _capi.DAU_OK and rb.max_abs_mu == want_b
        if bad == "nan":
            _assert_yardstick(rb, _yardstick(fam, 1), "nan, %s asked first: lane B" % first)
        seen_y.append(aa.as_bits(rb.outputs["y"]))
    assert np.array_equal(seen_y[0], seen_y[1])


# ---- 5. dau_conv_last_error is per thread --------------------------------------------------------------------------------------------
def test_last_error_is_per_thread():
    """Two threads make a refused call each on one plan -- a workspace declared one byte short, a null sigma; neither enqueues
    anything -- meet at a barrier and read dau_conv_last_error(): each finds its own message.  A third thread that has made no
    failing call reads an empty string."""
    from dau_conv import _capi
    fam = FAMILIES["split-k17"]
    plan = fam.plan()
    a = aa.Arena(_capi, plan, _inputs(fam, 0), fam.io, _capi.PASS_FORWARD, SKEW, 0x7B)
    torch.cuda.synchronize()
    barrier = threading.Barrier(3)
    seen, failures = {}, [None] * 3

    def call(sigma, short):
        return _capi.lib.dau_conv_forward(plan._h, a.stream, a.ptr("x"), a.ptr("w"), a.ptr("mu1"), a.ptr("mu2"), sigma, a.ptr("y"),
                                          a.ptr("workspace"), a.ws_bytes - short)

    def work(t):
        try:
            rc = None if t == 2 else call(a.ptr("sigma"), 1) if t == 0 else call(None, 0)
            barrier.wait(JOIN_SECONDS)
            seen[t] = (rc, _capi.lib.dau_conv_last_error())
        except BaseException as e:                            # noqa: B902
            failures[t] = e

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(3)]
    for th in threads:
        th.start()
    _join(threads, failures)
    assert seen[0][0] == _capi.DAU_INVALID_ARGUMENT and b"workspace too small" in seen[0][1], seen[0]
    assert seen[1][0] == _capi.DAU_INVALID_ARGUMENT and b"null argument" in seen[1][1], seen[1]
    assert seen[2] == (None, b""), seen[2]
    rep = a.finish(_capi.DAU_INVALID_ARGUMENT, ())           # and nothing was enqueued: not a byte of the arena has changed
    rep.assert_clean("refused calls")
    assert rep.untouched["workspace"] and rep.untouched["y"]


# ---- 6. the Python Plan's queries follow the calling thread --------------------------------------------------------------------------
def _dev(d, names):
    return [torch.from_numpy(np.ascontiguousarray(d[n])).cuda() for n in names]


def _two_threads_in_a_fixed_order(steps):
    """steps: [(thread 0 or 1, callable)] run strictly one after the other, each on its thread (and inside that thread's stream) ->
    the callables' results in order"""
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    turn = [threading.Event() for _ in range(len(steps) + 1)]
    out, failures = [None] * len(steps), [None, None]

    def work(t):
        try:
            with torch.cuda.stream(streams[t]):
                for i, (who, fn) in enumerate(steps):
                    if who == t:
                        assert turn[i].wait(JOIN_SECONDS), "step %d never got its turn" % i
                        try:
                            out[i] = fn()
                        finally:
                            turn[i + 1].set()
        except BaseException as e:                            # noqa: B902
            failures[t] = e
            for ev in turn:
                ev.set()

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for th in threads:
        th.start()
    turn[0].set()
    _join(threads, failures)
    return out


def test_python_plan_queries_follow_the_calling_thread():
    """dau_conv._capi.Plan is shared by every layer of a shape.  T1 calls plan.forward with a NaN offset on its stream, then T2 with
    clean offsets on its own; T1's plan.check_status() must still raise for T1's call, and T2's must return T2's max|mu|.  Likewise
    line_status() / dot_line_status(): each thread reads the counts of its own call."""
    from dau_conv import _capi
    fam = FAMILIES["split-k17"]
    plan = fam.plan()
    bad, clean = dict(_inputs(fam, 0)), _inputs(fam, 1)
    bad["mu1"] = bad["mu1"].copy()
    bad["mu1"].flat[0] = np.nan
    names = ("x", "w", "mu1", "mu2", "sigma")
    ta, tb = _dev(bad, names), _dev(clean, names)

    def check():
        try:
            return plan.check_status()
        except _capi.DAUConvError as e:
            return e

    out = _two_threads_in_a_fixed_order([(0, lambda: plan.forward(*ta)), (1, lambda: plan.forward(*tb)), (0, check), (1, check)])
    assert isinstance(out[2], _capi.FailedPreconditionError) and "NaN" in str(out[2]), "T1 asked about its NaN call and got %r" % (out[2],)
    assert out[3] == float(_max_abs_mu(clean)), out[3]
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    assert np.array_equal(aa.as_bits(out[1].cpu().numpy()), _yardstick(fam, 1)["y"])
    assert plan.last_status() in (None, float(_max_abs_mu(clean)))    # T1's check_status has reported the NaN: the plan's record of it is gone

    fam = FAMILIES["line"]
    plan = fam.plan()
    names = ("x", "dy", "w", "mu1", "mu2", "sigma")
    on, off = _dev(_inputs(fam, 0), names), _dev(_inputs(fam, 2), names)

    def step(t):
        x, dy, w, mu1, mu2, sigma = t
        return lambda: (plan.forward(x, w, mu1, mu2, sigma), plan.backward(x, dy, w, mu1, mu2, sigma))
    ask = lambda: (plan.line_status(), plan.dot_line_status())
    out = _two_threads_in_a_fixed_order([(0, step(on)), (1, step(off)), (0, ask), (1, ask)])
    assert out[2] == ((0, 4), (0, 4)), "T1's call lay on the line; it was told %r" % (out[2],)
    assert out[3] == ((len(OFF_LINE), 0), (len(OFF_LINE), 0)), "T2's call had %d units off the line; it was told %r" % (len(OFF_LINE), out[3])
    torch.cuda.synchronize()
    for t, lane in ((0, 0), (1, 2)):
        y, grads = out[t]
        got = dict(zip(("y", "dx") + PARAMS, (y,) + tuple(grads)))
        for n, v in got.items():
            assert np.array_equal(aa.as_bits(v.cpu().numpy()), _yardstick(fam, lane)[n]), "line lane %d %s" % (lane, n)
