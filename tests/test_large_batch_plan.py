"""CPU: the rows of tests/large_batch.py (activation tensors past 2^31 elements and 4 GiB; GPU: test_gpu_large_batch.py) at plan
level -- which limits each row's tensors cross (arithmetic on the shape), the batch slabs, members and workspace its plan reports,
that the image groups carrying a dy in the parameter-gradient call lie where they are meant to -- and the module's chunked
comparers on small CPU tensors against util.parity_error.  Plan creation needs no device; nothing is launched here."""
import numpy as np
import pytest
import torch

import large_batch as lb
import util

P = lb.P


def _plan(row):
    from dau_conv import _capi
    return _capi, lb.create_plan(_capi, row)


def test_the_shapes_cross_what_they_are_named_for():
    names = lambda row, which: [n for n, _ in lb.row_limits(lb.ROWS[row])[which]]
    # A: 1 075 773 440 elements of x
    assert 5360 * 64 * 56 * 56 == 1075773440 and 10704 * 64 * 56 * 56 == 2148335616
    assert names("r01_A_f32_exact", "x, dx") == ["2^30 elements", "2^32 bytes"] and names("r01_A_f32_exact", "y, dy") == []
    assert names("r02_A'_f32_exact", "y, dy") == ["2^30 elements", "2^32 bytes"] and names("r02_A'_f32_exact", "x, dx") == []
    assert names("r16_A_bf16_dense_bf16", "x, dx") == ["2^30 elements"]                       # 16-bit: 2.15 GB
    for row in ("r05_B_f16_split", "r07_B_f16_default", "r08_B_f16_split_one_slab", "r10_B_bf16_split", "r20_B_bf16_split_dot"):
        assert names(row, "x, dx") == ["2^30 elements", "2^31 elements", "2^32 bytes"] and names(row, "y, dy") == []
    for row in ("r06_B'_f16_split", "r09_B'_f16_exact_one_slab", "r12_B'_f16_exact_nhwc", "r12_B'_f16_exact_nchw"):
        assert names(row, "y, dy") == ["2^30 elements", "2^31 elements", "2^32 bytes"] and names(row, "x, dx") == []
    assert lb.ROWS["r18_many_f32_split"].shape[0] > lb.MAX_GRID_DIM and names("r18_many_f32_split", "x, dx") == []
    # whole images beyond the limit: ten of A beyond 2^30 elements, four of B (one image group) beyond 2^31
    per = 64 * 56 * 56
    assert 5360 - -(-(1 << 30) // per) == 10 and 10704 - -(-(1 << 31) // per) == 4
    # the staged fp32 copy of a whole B batch: past 2^33 bytes
    assert 10704 * per * 4 > 1 << 33


@pytest.mark.parametrize("rid", list(lb.ROWS))
def test_row_plan(rid):
    row = lb.ROWS[rid]
    capi, plan = _plan(row)
    lb.assert_phase(row)
    info, want = plan.info, row.expect
    N = row.shape[0]
    assert info["batch_slab_gather"] == want["slab_gather"] and info["batch_slab_dot"] == want["slab_dot"], info
    assert info["gather_dense_split"] == want["split"], bin(info["gather_dense_split"])
    assert info["algo_forward"] == info["algo_backward"] == want.get("algo_forward", capi.ALGO_TILED)
    assert (info["gather_dense_bf16"] == 2) == row.grads16 and info["gather_dense_bf16"] == want.get("dense_bf16", 0)
    assert info["offset_bucket"] == want.get("bucket", 4)
    assert info["dot_windows"] == want.get("dot_windows", 0 if row.algo == capi.ALGO_DIRECT else 1)
    assert info["gather_windows"] == want.get("gather_windows", 0 if row.algo == capi.ALGO_DIRECT else 1)
    if row.k == 65:
        assert info["bucket_sets"] == 1          # static: every call runs the bucket-32 set, the only one with offset windows
    limits = {key: [n for n, _ in v] for key, v in lb.row_limits(row).items()}
    assert limits == {"x, dx": want["lim_x"], "y, dy": want["lim_y"]}, limits
    ws = [round(plan.workspace_bytes(w) / 1e9, 2) for w in (capi.PASS_FORWARD, capi.PASS_BACKWARD)]
    assert ws == [want["ws_fwd"], want["ws_bwd"]], ws
    if row.budget == "24" and rid.startswith(("r08", "r09")):
        assert info["batch_slab_gather"] == N
    # K: whole groups inside the batch; the first and the last; the last one wholly beyond every limit the row crosses; the group
    # that holds the first element past a limit does hold it; both sides of every slab boundary, none of them cut by it
    K = lb.key_groups(row, info["batch_slab_gather"], info["batch_slab_dot"])
    assert K == sorted(set(K)) and K[0] == 0 and K[-1] == N // P - 1 and N % P == 0
    assert K == lb.key_groups(row, info["batch_slab_gather"], info["batch_slab_dot"])          # seeded
    crossed = 0
    for per, key in zip(lb.per_image(row), ("x, dx", "y, dy")):
        for name, el in lb.row_limits(row)[key]:
            crossed += 1
            assert (N - P) * per >= el, "%s: the last image group is cut by %s of %s" % (rid, name, key)
            g = el // (P * per)
            assert g in K and g * P * per <= el < (g + 1) * P * per
    assert crossed or N > lb.MAX_GRID_DIM, "%s crosses nothing" % rid
    slabs = 0
    for slab in (info["batch_slab_gather"], info["batch_slab_dot"]):
        assert slab % P == 0, "a slab boundary cuts an image group"
        for b in range(slab, N, slab):
            slabs += 1
            assert b // P - 1 in K and b // P in K
    middle = [g for g in K if 0 < g < N // P - 1]
    assert len(middle) >= 3 and len(K) <= 2 + 2 * crossed + 2 * slabs + 3 + 2


def test_nhwc_rows_are_their_twins_plan():
    for rid in ("r11_A_f32_split_nhwc", "r12_B'_f16_exact_nhwc"):
        row = lb.ROWS[rid]
        capi, plan = _plan(row)
        _, twin = _plan(lb.nchw_twin(row))
        assert plan.io_layout == "NHWC" and twin.io_layout == "NCHW" and plan.info == twin.info
        assert [plan.workspace_bytes(w) for w in (1, 2)] == [twin.workspace_bytes(w) for w in (1, 2)]
    # the twins are rows of their own
    assert lb.nchw_twin(lb.ROWS["r11_A_f32_split_nhwc"]) is lb.ROWS["r03_A_f32_split_r3"]
    assert lb.nchw_twin(lb.ROWS["r12_B'_f16_exact_nhwc"]) is lb.ROWS["r12_B'_f16_exact_nchw"]


def test_rows_are_created_under_their_own_budget(monkeypatch):
    monkeypatch.setenv(lb.BUDGET, "0.5")
    capi, plan = _plan(lb.ROWS["r18_many_f32_exact"])
    assert plan.info["batch_slab_gather"] == 70000
    import os
    assert os.environ[lb.BUDGET] == "0.5"


def test_byte_offsets():
    row = lb.ROWS["r05_B_f16_split"]
    assert lb.byte_offset(10700, 0, 0, 0, row, 64) == 10700 * 64 * 56 * 56 * 2 > 1 << 32
    assert lb.byte_offset(1, 2, 3, 4, row, 64) == (((1 * 64 + 2) * 56 + 3) * 56 + 4) * 2
    nhwc = lb.ROWS["r12_B'_f16_exact_nhwc"]
    assert lb.byte_offset(1, 2, 3, 4, nhwc, 64) == (((1 * 56 + 3) * 56 + 4) * 64 + 2) * 2


# ---- the comparers ---------------------------------------------------------------------------------------------------------------

def _tiled(rs, groups, C=3, H=5, W=7, dtype=np.float32, noise=1e-6):
    want = rs.randn(P, C, H, W)
    got = (np.tile(want, (groups, 1, 1, 1)) * (1 + noise * rs.randn(groups * P, C, H, W))).astype(dtype)
    return got, want


@pytest.mark.parametrize("chunk", [1, 400, 1000, 1 << 24])       # one group per chunk, a ragged last chunk, everything at once
@pytest.mark.parametrize("rel, floor, noise", [(1e-4, 1e-6, 1e-6), (1e-4, 1e-6, 1e-3), (2e-2, 4e-3, 1e-2)])
def test_parity_chunked_is_parity_error(chunk, rel, floor, noise):
    rs = np.random.RandomState(3)
    got, want = _tiled(rs, 7, noise=noise)
    ref = util.parity_error(got, np.tile(want, (7, 1, 1, 1)), rel, floor)
    res = lb.parity_chunked(torch.from_numpy(got), torch.from_numpy(want), rel, floor, chunk_elems=chunk)
    assert res.violation == ref and res.nans == 0            # to the last bit
    assert (res.first is None) == (ref <= 0)
    if ref > 0:                                              # the first element over the bar, in [N, C, H, W] order
        g, w = got.astype(np.float64), np.tile(want, (7, 1, 1, 1))
        over = np.abs(g - w) - (rel * np.abs(w) + floor * np.abs(want).max() + 1e-12) > 0
        assert res.first == tuple(int(i) for i in np.unravel_index(np.argmax(over), over.shape))
        assert res.gotv == float(got[res.first]) and res.wantv == w[res.first]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_parity_chunked_on_strided_16_bit_arrays(dtype):
    """an NHWC array seen as [N, C, H, W], in the storage formats of the rows"""
    rs = np.random.RandomState(4)
    got, want = _tiled(rs, 5, noise=0.0)
    mem = torch.from_numpy(got).to(dtype).permute(0, 2, 3, 1).contiguous()
    logical = mem.permute(0, 3, 1, 2)
    ref = util.parity_error(logical.float().numpy(), np.tile(want, (5, 1, 1, 1)), 2e-2, 4e-3)
    res = lb.parity_chunked(logical, torch.from_numpy(want), 2e-2, 4e-3, chunk_elems=250)
    assert res.violation == ref and ref <= 0 and res.first is None


def _one_ulp_over(want, idx, rel=1e-4, floor=1e-6):
    """the smallest float32 above want[idx] whose distance exceeds the bar, and the largest one within it"""
    w = want[idx]
    tol = rel * abs(w) + floor * np.abs(want).max() + 1e-12
    v = np.float32(w + tol)
    while abs(np.float64(v) - w) <= tol:
        v = np.nextafter(v, np.float32(np.inf))
    below = np.nextafter(v, np.float32(-np.inf))
    assert abs(np.float64(below) - w) <= tol < abs(np.float64(v) - w)
    return v, below


@pytest.mark.parametrize("where", [(0, 0, 0, 0), (13, 1, 2, 3), (27, 2, 4, 6)])      # first chunk, a middle one, the last element
def test_a_planted_error_one_ulp_over_the_bar_fails(where):
    rs = np.random.RandomState(5)
    got, want = _tiled(rs, 7, noise=0.0)
    want32 = want.astype(np.float32).astype(np.float64)      # got == want exactly but for the planted element
    got = np.tile(want32, (7, 1, 1, 1)).astype(np.float32)
    over, within = _one_ulp_over(want32, (where[0] % P,) + where[1:])
    got[where] = within
    res = lb.parity_chunked(torch.from_numpy(got), torch.from_numpy(want32), chunk_elems=500)
    assert res.violation <= 0 and res.first is None
    got[where] = over
    res = lb.parity_chunked(torch.from_numpy(got), torch.from_numpy(want32), chunk_elems=500)
    assert res.violation > 0 and res.first == where and res.nans == 0
    assert res.violation == util.parity_error(got, np.tile(want32, (7, 1, 1, 1)))
    row = lb.ROWS["r01_A_f32_exact"]._replace(shape=(28, 3, 3, 1, 5, 7))
    with pytest.raises(AssertionError, match=r"first at image %d \(c %d, y %d, x %d\), byte offset %d:" % (
            where + (lb.byte_offset(*where, row=row, channels=3),))):
        lb.assert_tensor(torch.from_numpy(got), want32, row, 3, "y", bits=False)


@pytest.mark.parametrize("where", [(0, 0, 0, 0), (13, 1, 2, 3), (27, 2, 4, 6)])
def test_a_planted_nan_fails(where):
    rs = np.random.RandomState(6)
    got, want = _tiled(rs, 7, noise=0.0)
    got[where] = np.nan
    res = lb.parity_chunked(torch.from_numpy(got), torch.from_numpy(want), chunk_elems=500)
    assert res.nans == 1 and res.first == where
    assert res.violation <= 0                                # the rest is within the bar: the NaN is reported apart
    row = lb.ROWS["r01_A_f32_exact"]._replace(shape=(28, 3, 3, 1, 5, 7))
    with pytest.raises(AssertionError, match="1 NaN.*first at image %d " % where[0]):
        lb.assert_tensor(torch.from_numpy(got), want, row, 3, "y", bits=False)
    # an array left at its 0xFF fill fails in every element
    poisoned = lb._poison(torch.empty(28, 3, 5, 7))
    assert lb.parity_chunked(poisoned, torch.from_numpy(want), chunk_elems=500).nans == poisoned.numel()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_bit_and_zero_checks(dtype):
    rs = np.random.RandomState(7)
    base = torch.from_numpy(rs.randn(P, 3, 5, 7).astype(np.float32)).to(dtype)
    mem = base.repeat(9, 1, 1, 1)
    ge = P * 3 * 5 * 7
    for chunk in (1, 3 * ge, 1 << 26):
        assert lb.first_group_differing(mem, ge, chunk) is None
    mem[22, 1, 2, 3] = -mem[22, 1, 2, 3]                     # one sign bit, in group 5
    mem[30, 0, 0, 0] = 0.5
    for chunk in (1, 3 * ge, 1 << 26):
        assert lb.first_group_differing(mem, ge, chunk) == (5, (2 * 3 * 5 + 1 * 5 + 2) * 7 + 3)
    # +0 against -0: other bits
    z = torch.zeros(8, 1, 2, 2, dtype=dtype)
    z[5, 0, 1, 1] = -0.0
    assert lb.first_group_differing(z, 4 * 4) == (1, 7)
    # ... but zero by value
    assert lb.first_group_nonzero(z, 4 * 4, ()) is None
    z[5, 0, 1, 0] = float("nan")
    assert lb.first_group_nonzero(z, 4 * 4, ()) == (1, 6) and lb.first_group_nonzero(z, 4 * 4, (1,)) is None
    mem = torch.zeros(36, 3, 5, 7, dtype=dtype)
    mem[8:12] = base
    mem[35, 2, 4, 6] = 1e-7 if dtype != torch.float16 else 6e-8          # the smallest things count
    for chunk in (1, 3 * ge, 1 << 26):
        assert lb.first_group_nonzero(mem, ge, (2,), chunk) == (8, ge - 1)
        assert lb.first_group_nonzero(mem, ge, (2, 8), chunk) is None
    assert lb._locate(lb.ROWS["r05_B_f16_split"], 64, 2674, 5) == "image 10696, byte offset %d" % ((2674 * 4 * 64 * 56 * 56 + 5) * 2)
