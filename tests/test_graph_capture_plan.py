"""CPU: what graph capture of a DAU layer needs of the library and of the plan cache, as far as it can be asked without a device --
the sigma-support entry point (declared, exported, its argument checks, its answer for a plan without a pinned mirror), its binding,
and the pinning of the plans a captured call has used: the eviction skips them until release_captured_plans().  The captures
themselves run in tests/test_gpu_graph_capture.py."""
import ctypes
import gc
import importlib
import os
import re
import weakref

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dau_conv.h")

from dau_conv import _capi   # noqa: E402

dc = importlib.import_module("dau_conv.dau_conv")            # (the package attribute of that name is the op function)


def test_sigma_status_is_declared_and_exported():
    src = open(HEADER).read()
    assert re.search(r"DAU_API\s+int\s+dau_conv_sigma_status\s*\(\s*const\s+dau_conv_plan\s*\*\s*plan\s*,\s*int32_t\s*\*\s*needed_out\s*,"
                     r"\s*int32_t\s*\*\s*planned_out\s*,\s*int32_t\s*\*\s*worst_needed_out\s*\)", src)
    assert hasattr(_capi.lib, "dau_conv_sigma_status")
    assert _capi.lib.dau_conv_abi_version() == 4             # an addition: the version stays, as with the line-status entries
    # the header's "HIP graphs" paragraph says what a replaying caller must know
    graphs = src[src.index("HIP graphs."):src.index("#ifndef DAU_CONV_H_")]
    assert "dau_conv_sigma_status" in graphs and "frozen" in graphs


def test_sigma_status_argument_checks_and_a_plan_without_a_device():
    """Null arguments are refused; a plan without a pinned mirror answers (0, planned, 0).  On a machine with a device the plan has a
    mirror that no call has written yet: the same answer."""
    for sigma, k in ((0.5, 7), (0.8, 9), (0.3, 5)):
        plan = _capi.Plan(2, 3, 4, 2, 8, 9, max_kernel_size=9, sigma_hint=sigma)
        assert plan.sigma_status() == (0, k, 0)
        assert plan.sigma_status() == (0, k, 0)              # asking clears nothing that was not there
    v = [ctypes.c_int32(-1) for _ in range(3)]
    ref = [ctypes.byref(c) for c in v]
    fn = _capi.lib.dau_conv_sigma_status
    assert fn(None, *ref) == _capi.DAU_INVALID_ARGUMENT
    for missing in range(3):
        args = list(ref)
        args[missing] = None
        assert fn(plan._h, *args) == _capi.DAU_INVALID_ARGUMENT
        assert b"null" in _capi.lib.dau_conv_last_error()
    assert [c.value for c in v] == [-1, -1, -1]              # a refused call writes nothing
    assert fn(plan._h, *ref) == _capi.DAU_OK and [c.value for c in v] == [0, 5, 0]
    assert plan.last_status() is None                        # the offset status is untouched by it


def test_the_capture_surface_exists():
    import dau_conv
    assert callable(_capi.Plan.sigma_status) and callable(dau_conv.release_captured_plans)
    assert "release_captured_plans" in dc.__all__
    assert isinstance(dc._PINNED, set) and callable(dc._pin)
    cpu = torch.device("cpu")
    assert _capi.capturing(cpu) is False                     # no device, no capture: today's path
    plan = _capi.Plan(2, 3, 4, 2, 8, 9)
    assert plan.captured is False
    for query in (plan.check_status, plan.outlier_status, plan.line_status, plan.dot_line_status):
        try:
            query()
        except _capi.FailedPreconditionError as e:           # (no call yet: there is no workspace to read)
            assert "before any" in str(e)
        else:
            raise AssertionError("%s answered without a call" % query.__name__)


def _plan_of(h, w4):
    st = dc._settings(torch.full((1,), 0.5), num_output=4, kernel_size=9)
    dev = "cuda" if torch.cuda.is_available() else "cpu"     # (the plan is made for the input's device; no kernel runs either way)
    return dc._get_plan(torch.zeros(2, 3, h, 9, device=dev), w4.to(dev), st)


def test_a_pinned_plan_survives_the_eviction_until_it_is_released():
    dc._PLANS.clear()
    dc._PINNED.clear()
    w4 = torch.zeros(1, 3, 2, 4)
    try:
        pinned = _plan_of(8, w4)
        key = pinned._cache_key
        assert dc._PLANS[key] is pinned
        dc._pin(pinned)
        assert dc._PINNED == {key}
        alive = weakref.ref(pinned)
        del pinned
        flood = lambda first: [_plan_of(h, w4) and None for h in range(first, first + dc._PLAN_CACHE_MAX + 1)]
        flood(9)                                             # 65 further plans enter the cache
        gc.collect()
        assert alive() is not None and key in dc._PLANS and next(iter(dc._PLANS)) == key
        assert len(dc._PLANS) == dc._PLAN_CACHE_MAX + 1      # the pinned plan does not count against the bound
        assert _plan_of(8, w4) is alive()                    # and is still the plan of its shape
        dc.release_captured_plans()
        assert not dc._PINNED and len(dc._PLANS) == dc._PLAN_CACHE_MAX
        flood(200)
        gc.collect()
        assert alive() is None and key not in dc._PLANS
        # a cache emptied by hand takes its pins with it: the bound is the old one again, and a new plan of a pinned key is not pinned
        again = _plan_of(8, w4)
        dc._pin(again)
        dc._PLANS.clear()
        flood(9)
        assert not dc._PINNED and len(dc._PLANS) == dc._PLAN_CACHE_MAX
        dc._PLANS.clear()
        # a plan made outside the cache has no key: pinning it is a no-op
        dc._pin(_capi.Plan(2, 3, 4, 2, 8, 9))
        assert not dc._PINNED
    finally:
        dc._PINNED.clear()
        dc._PLANS.clear()


def test_the_eviction_order_without_pins_is_least_recently_used():
    dc._PLANS.clear()
    dc._PINNED.clear()
    w4 = torch.zeros(1, 3, 2, 4)
    try:
        plans = [_plan_of(h, w4) for h in range(8, 8 + dc._PLAN_CACHE_MAX)]
        keys = [p._cache_key for p in plans]
        assert list(dc._PLANS) == keys
        assert _plan_of(8, w4) is plans[0]                   # a hit moves the plan to the young end
        assert list(dc._PLANS) == keys[1:] + keys[:1]
        _plan_of(500, w4)                                    # one more: the oldest, now keys[1], goes
        assert len(dc._PLANS) == dc._PLAN_CACHE_MAX and keys[1] not in dc._PLANS and keys[0] in dc._PLANS
        _plan_of(501, w4)
        assert keys[2] not in dc._PLANS and keys[3] in dc._PLANS
        # with one plan pinned in the middle of the order the others still leave oldest first
        dc._pin(plans[3])
        _plan_of(502, w4)
        assert keys[3] in dc._PLANS and keys[4] in dc._PLANS and len(dc._PLANS) == dc._PLAN_CACHE_MAX + 1
        _plan_of(503, w4)
        assert keys[3] in dc._PLANS and keys[4] not in dc._PLANS and keys[5] in dc._PLANS
    finally:
        dc._PINNED.clear()
        dc._PLANS.clear()
