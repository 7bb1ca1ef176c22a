"""GPU: activation tensors past 2^30 / 2^31 elements and 2^32 bytes through every member (rows and checks: tests/large_batch.py; the
plans of the rows: tests/test_large_batch_plan.py).  Each row runs forward, the input gradient and the parameter gradients of a
sparse dy through the C ABI with buffers of its own, and checks whole tensors on the device: against the oracle's four base images
at the bar of util.assert_parity, no NaN left of the 0xFF fill, every image bit-identical to its base image's, dx exactly zero
where dy is.  A wrapped index at these sizes rarely faults -- it reads or writes another image -- so the first failing image and
its byte offset are what a failure reports.

A row first compares torch.cuda.mem_get_info() with what it will hold plus 10 % and skips if the card does not have it (a row needs
19 - 51 GB, the last one 95 GB); on an otherwise idle MI355X nothing skips."""
import pytest
import torch

import large_batch as lb

pytestmark = pytest.mark.gpu


def _run(rid):
    from dau_conv import _capi
    row = lb.ROWS[rid]
    plan = lb.create_plan(_capi, row)
    need = int(lb.memory_needed(_capi, row, plan) * 1.1)
    del plan
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("%s needs %d bytes of device memory (its tensors, workspace and 10 %%), %d are free" % (rid, need, free))
    return _capi, row, lb.run_row(_capi, row)


@pytest.mark.parametrize("rid", [r for r in lb.ROWS if not lb.is_nhwc(lb.ROWS[r])])
def test_large_batch_row(rid):
    capi, row, rec = _run(rid)
    if row.budget == "24" and not row.grads16:
        assert rec["batch_slab_gather"] == row.shape[0]      # one gather slab: the offsets inside the kernels cross


@pytest.mark.parametrize("rid", [r for r in lb.ROWS if lb.is_nhwc(lb.ROWS[r])])
def test_large_batch_row_nhwc(rid):
    """((n H + y) W + x) C + c: the same checks on NHWC arrays, and the bits of the NCHW call of the same plan"""
    capi, row, rec = _run(rid)
    got = lb.first_group(capi, row)
    ref = lb.first_group(capi, lb.nchw_twin(row))            # rows 3 and 12-NCHW: they have run, in a whole-module run
    for key in ("y", "dx") + lb.GRADS:
        differ = int((got[key] != ref[key]).sum())
        assert differ == 0, "%s %s: %d of %d values of the first image group differ from the NCHW call's" % (rid, key, differ, ref[key].size)
