"""Activation tensors past 2^31 elements and 4 GiB through the C ABI (helper module of test_large_batch_plan.py and
test_gpu_large_batch.py; not a test).

A row is one plan at a batch size whose x / dx or y / dy leave 30, 31 or 32 bits of element offset, or 32 or 33 bits of byte offset.
Nothing of that size exists on the host: x holds P = 4 distinct base images tiled over the batch (x[n] = base[n % P]), the oracle
runs on those P images, and every check of a whole tensor runs on the device in chunks of whole image groups.  P * C * H * W has an
odd prime factor for both channel counts, so it divides no power of two: a load or store whose offset wrapped by 2^31, 2^32 or 2^33
elements or bytes lands at another phase of another base image -- it cannot land on identical data.

The library is called through dau_conv._capi.lib with buffers this module owns: outputs and a workspace of exactly
dau_conv_workspace_bytes, all filled with 0xFF bytes (a NaN in all three formats) before the call, the workspace freed after the row
(Plan.forward / Plan.backward would keep their grow-only shared workspace of up to 19 GB for the rest of the session).

Checks of one row (run_row): y and dx of the tiled call against the oracle's P images at the bar util.assert_parity has for the
format, no NaN left (every element was written), y[n] / dx[n] bit-identical to image n % P; then a backward call whose dy is zero but
on a set K of image groups (key_groups: first, last, the groups holding the first element past each limit, both sides of every slab
boundary, three seeded ones), each with a dy of its own: the parameter gradients against the float64 sum of the oracle's over those
groups, dx exactly zero outside K and at the bar inside.
"""
import ctypes
import json
import os
import time
from collections import OrderedDict, namedtuple

import numpy as np

import util

DEVICE = "cuda"           # test_large_batch_plan.py runs the comparers on CPU tensors; they take the device of what they are given
P = 4                     # distinct base images
BUDGET = "DAU_WORKSPACE_BUDGET_GB"

from dau_conv import _capi as _flags          # the flag values only; the calls go through the capi module the caller hands in

I, IO_BF16, DENSE_BF16, SPLIT, NO_SPLIT = (_flags.FLAG_USE_INTERPOLATION, _flags.FLAG_IO_BF16, _flags.FLAG_DENSE_BF16,
                                           _flags.FLAG_DENSE_SPLIT_F16, _flags.FLAG_NO_DENSE_SPLIT)
IO_F16, OUTLIERS, NHWC, STATIC = _flags.FLAG_IO_F16, _flags.FLAG_DENSE_SPLIT_OUTLIERS, _flags.FLAG_IO_NHWC, _flags.FLAG_STATIC_BUCKET
ALGO_AUTO, ALGO_DIRECT = _flags.ALGO_AUTO, _flags.ALGO_DIRECT
ESIZE = {"f32": 4, "f16": 2, "bf16": 2}
IOFLAG = {"f32": 0, "f16": IO_F16, "bf16": IO_BF16}
ELEMENT_LIMITS = (30, 31, 32)      # 2^b elements
BYTE_LIMITS = (32, 33)             # 2^b bytes
MAX_GRID_DIM = 65535               # images: more than that cannot be one grid dimension

# id, (N, S, F, G, H, W), k, offset range, storage, plan flags besides USE_INTERPOLATION and the storage flag, algo,
# DAU_WORKSPACE_BUDGET_GB (None: the default), corner (two units at +-corner: the call belongs to that radius' member), outlier (one
# unit at 3.5), calls (2: the second call finds the first call's outputs and workspace), bf16 bar for the parameter gradients,
# expect: what test_large_batch_plan.py asserts of the plan
Row = namedtuple("Row", "id shape k m io flags algo budget corner outlier calls grads16 expect")

E30, E31, B32 = "2^30 elements", "2^31 elements", "2^32 bytes"      # the limits a row's x / dx (lim_x) or y / dy (lim_y) cross
A = (5360, 64, 8, 2, 56, 56)       # x, dx: 1 075 773 440 elements -- past 2^30 elements, past 2^32 bytes in fp32; ten images beyond
A_ = (5360, 8, 64, 2, 56, 56)      # y, dy cross
B = (10704, 64, 8, 2, 56, 56)      # x, dx: 2 148 335 616 elements -- past 2^31 elements, past 2^32 bytes in 16-bit storage; four beyond
B_ = (10704, 8, 64, 2, 56, 56)
A3 = (5360, 64, 8, 3, 56, 56)
A9 = (5360, 64, 8, 9, 56, 56)      # nine units: the bucket-32 gather-sum takes four offset windows
MANY = (70000, 7, 7, 2, 8, 8)      # more than 65535 images (seven channels: 8 x 8 maps of eight would be a power of two)


def _row(id, shape, io="f32", flags=0, k=9, m=3.0, algo=ALGO_AUTO, budget=None, corner=3.0, outlier=False, calls=1, grads16=False,
         **expect):
    return Row(id, shape, k, m, io, flags, algo, budget, corner, outlier, calls, grads16, expect)


ROWS = OrderedDict((r.id, r) for r in (
    # exact gather and exact gather-dot, 4 GiB byte offsets
    _row("r01_A_f32_exact", A, flags=NO_SPLIT, lim_x=[E30, B32], lim_y=[], slab_gather=5360, slab_dot=2680, split=0, ws_fwd=7.38, ws_bwd=10.98),
    _row("r02_A'_f32_exact", A_, flags=NO_SPLIT, lim_x=[], lim_y=[E30, B32], slab_gather=5360, slab_dot=2680, split=0, ws_fwd=0.92, ws_bwd=18.88),
    # two-limb members: staging, GEMM epilogue, per-image maxima; radius 3 and radius 4
    _row("r03_A_f32_split_r3", A, flags=SPLIT, lim_x=[E30, B32], lim_y=[], slab_gather=5360, slab_dot=2680, split=0b11100, ws_fwd=7.38, ws_bwd=11.46),
    _row("r04_A'_f32_split_r4", A_, flags=SPLIT, m=3.99, corner=3.99, lim_x=[], lim_y=[E30, B32], slab_gather=5360, slab_dot=2680, split=0b11100, ws_fwd=1.41,
         ws_bwd=18.88),
    # 2^31 elements across slab bases
    _row("r05_B_f16_split", B, "f16", SPLIT, lim_x=[E30, E31, B32], lim_y=[], slab_gather=5352, slab_dot=2676, split=0b11100, ws_fwd=7.37, ws_bwd=11.45),
    _row("r06_B'_f16_split", B_, "f16", SPLIT, lim_x=[], lim_y=[E30, E31, B32], slab_gather=5352, slab_dot=2676, split=0b11100, ws_fwd=1.40, ws_bwd=18.85),
    # whatever the default plan picks: the exact members (G = 2 pays for no dense radius; the gather-dot runs in two slabs, and the
    # two-limb gather-dot takes whole batches only)
    _row("r07_B_f16_default", B, "f16", lim_x=[E30, E31, B32], lim_y=[], slab_gather=5352, slab_dot=2676, split=0, ws_fwd=7.37, ws_bwd=10.96),
    # one gather slab: in-kernel element offsets past 2^31, a staged copy past 2^33 bytes
    _row("r08_B_f16_split_one_slab", B, "f16", SPLIT, budget="24", lim_x=[E30, E31, B32], lim_y=[], slab_gather=10704, slab_dot=5352, split=0b11100, ws_fwd=14.73,
         ws_bwd=22.89),
    _row("r09_B'_f16_exact_one_slab", B_, "f16", NO_SPLIT, budget="24", lim_x=[], lim_y=[E30, E31, B32], slab_gather=10704, slab_dot=5352, split=0, ws_fwd=1.84,
         ws_bwd=37.71),
    # bfloat16 storage on the two-limb gather-sum members
    _row("r10_B_bf16_split", B, "bf16", SPLIT, lim_x=[E30, E31, B32], lim_y=[], slab_gather=5352, slab_dot=2676, split=0b11100, ws_fwd=7.37, ws_bwd=11.45),
    # ((n H + y) W + x) C + c; the bits of the NCHW call
    _row("r11_A_f32_split_nhwc", A, flags=SPLIT | NHWC, lim_x=[E30, B32], lim_y=[], slab_gather=5360, slab_dot=2680, split=0b11100, ws_fwd=7.38, ws_bwd=11.46),
    _row("r12_B'_f16_exact_nchw", B_, "f16", NO_SPLIT, lim_x=[], lim_y=[E30, E31, B32], slab_gather=5352, slab_dot=2676, split=0,
         ws_fwd=0.92, ws_bwd=18.85),                       # (the NCHW call whose bits row 12 must have; row 11's is row 3)
    _row("r12_B'_f16_exact_nhwc", B_, "f16", NO_SPLIT | NHWC, lim_x=[], lim_y=[E30, E31, B32], slab_gather=5352, slab_dot=2676, split=0, ws_fwd=0.92, ws_bwd=18.85),
    # the ring pass and its N F H W partial sums
    _row("r13_A'_f32_outliers", A_, flags=SPLIT | OUTLIERS, outlier=True, lim_x=[], lim_y=[E30, B32], slab_gather=5360, slab_dot=2680, split=0b111100, ws_fwd=5.62,
         ws_bwd=18.88),
    # larger halos
    _row("r14_A_f32_k17", A, flags=NO_SPLIT, k=17, m=7.0, corner=None, lim_x=[E30, B32], lim_y=[], slab_gather=2680, slab_dot=2680, split=0, ws_fwd=7.38,
         ws_bwd=11.36, bucket=8),
    # bucket 32: the binned gather-dot in offset windows (sgroup) and, with nine units, the gather-sum in four offset windows, whose
    # passes accumulate into y / dx: the second call finds the first call's outputs.  DAU_FLAG_STATIC_BUCKET: a plan that selects per
    # call would run its bucket-20 set (one pass, no windows) for offsets within +-20 from the second call on
    _row("r15_A_f32_k65", A, flags=STATIC, k=65, m=20.0, corner=None, calls=2, lim_x=[E30, B32], lim_y=[], slab_gather=1072, slab_dot=1340,
         split=0, ws_fwd=11.42, ws_bwd=13.07, bucket=32, dot_windows=16, gather_windows=1),
    _row("r15_A9_f32_k65_windows", A9, flags=STATIC, k=65, m=20.0, corner=None, calls=2, lim_x=[E30, B32], lim_y=[], slab_gather=1340,
         slab_dot=1340, split=0, ws_fwd=11.42, ws_bwd=13.30, bucket=32, dot_windows=16, gather_windows=4),
    # bf16-product members.  The dense parameter gradients (k_dense_wgrad.hip) take whole batches only: at the default budget the
    # gather-dot of this shape runs in two slabs and the plan does not hold them, so the row raises the budget
    _row("r16_A_bf16_dense_bf16", A3, "bf16", DENSE_BF16, budget="24", grads16=True, lim_x=[E30], lim_y=[], slab_gather=5360, slab_dot=5360, split=0,
         dense_bf16=2, ws_fwd=7.38, ws_bwd=21.04),
    # the direct kernels
    _row("r17_A_f32_direct", A, algo=ALGO_DIRECT, lim_x=[E30, B32], lim_y=[], slab_gather=5360, slab_dot=2680, split=0, algo_forward=ALGO_DIRECT, ws_fwd=4.30,
         ws_bwd=17.75),
    # more than 65535 images
    _row("r18_many_f32_split", MANY, flags=SPLIT, lim_x=[], lim_y=[], slab_gather=70000, slab_dot=70000, split=0b11100, ws_fwd=1.76, ws_bwd=8.93),
    _row("r18_many_f32_exact", MANY, flags=NO_SPLIT, lim_x=[], lim_y=[], slab_gather=70000, slab_dot=70000, split=0, ws_fwd=1.76, ws_bwd=8.93),
    # the two-limb gather-dot (k_split_dot.hip) takes whole batches only, so no row above runs it: these two raise the budget until
    # the gather-dot is one slab -- two-limb error staging across 4 GiB, one-limb (bfloat16) error staging past 2^31 elements.
    # No field of dau_conv_plan_info names that member: that the plan holds it shows in the backward workspace alone (the exact
    # gather-dot in one slab needs 21.52 GB for A; these figures are the split member's)
    _row("r19_A_f32_split_dot", A, flags=SPLIT, budget="48", lim_x=[E30, B32], lim_y=[], slab_gather=5360, slab_dot=5360, split=0b11100, ws_fwd=7.38, ws_bwd=40.63),
    _row("r20_B_bf16_split_dot", B, "bf16", SPLIT, budget="100", lim_x=[E30, E31, B32], lim_y=[], slab_gather=10704, slab_dot=10704, split=0b11100, ws_fwd=14.73,
         ws_bwd=79.55),
))


def plan_flags(row):
    return I | IOFLAG[row.io] | row.flags


def is_nhwc(row):
    return bool(row.flags & NHWC)


def nchw_twin(row):
    """the row of ROWS that is this one without DAU_FLAG_IO_NHWC: same inputs, same plan in everything but addresses"""
    (twin,) = [r for r in ROWS.values() if _first_key(r) == _first_key(row._replace(flags=row.flags & ~NHWC))]
    return twin


def bar(row, grads=False):
    """(rel, floor) of util.assert_parity: its fp32 defaults; 2e-2 / 4e-3 for y and dx in 16-bit storage (tests/test_gpu_bf16.py) and
    for the parameter gradients of the bf16-product dense forms (tests/test_gpu_dense_bf16.py)"""
    if (grads and row.grads16) or (not grads and row.io != "f32"):
        return 2e-2, 4e-3
    return 1e-4, 1e-6


# ---- arithmetic on the shape ----------------------------------------------------------------------------------------------------

def per_image(row):
    """elements of one image of x / dx and of y / dy"""
    N, S, F, G, H, W = row.shape
    return S * H * W, F * H * W


def limits_crossed(numel, esize):
    """-> [(name, index of the first element past the limit)] of the limits a tensor of numel elements crosses"""
    out = [("2^%d elements" % b, 1 << b) for b in ELEMENT_LIMITS if numel > 1 << b]
    out += [("2^%d bytes" % b, (1 << b) // esize) for b in BYTE_LIMITS if numel * esize > 1 << b]
    return out


def row_limits(row):
    """-> {"x, dx": [...], "y, dy": [...]} of limits_crossed"""
    N = row.shape[0]
    px, py = per_image(row)
    return {"x, dx": limits_crossed(N * px, ESIZE[row.io]), "y, dy": limits_crossed(N * py, ESIZE[row.io])}


def assert_phase(row):
    """P * C * H * W divides no power of two, for both channel counts, and the batch is whole groups"""
    assert row.shape[0] % P == 0, row.id
    for per in per_image(row):
        odd = P * per
        while odd % 2 == 0:
            odd //= 2
        assert odd > 1, "%s: a group of %d images is %d elements, a power of two: a wrapped offset could land on identical data" % (
            row.id, P, P * per)


def key_groups(row, slab_gather, slab_dot, seed=20):
    """K: the image groups (of P images) that carry a dy in the parameter-gradient call, sorted"""
    N = row.shape[0]
    ng = N // P
    K = {0, ng - 1}
    for per, crossed in zip(per_image(row), (row_limits(row)["x, dx"], row_limits(row)["y, dy"])):
        K.update(el // per // P for _, el in crossed)
    if N > MAX_GRID_DIM:
        K.update((MAX_GRID_DIM // P, (MAX_GRID_DIM + 1) // P))
    for slab in (slab_gather, slab_dot):
        for b in range(slab, N, slab):
            K.update(((b - 1) // P, b // P))
    rs = np.random.RandomState(seed)
    middle = [g for g in range(1, ng - 1) if g not in K]
    K.update(int(g) for g in rs.choice(middle, 3, replace=False))
    return sorted(K)


def byte_offset(n, c, y, x, row, channels):
    """of element (n, c, y, x) of an activation tensor of `channels` channels in the row's layout and storage"""
    N, S, F, G, H, W = row.shape
    el = ((n * H + y) * W + x) * channels + c if is_nhwc(row) else ((n * channels + c) * H + y) * W + x
    return el * ESIZE[row.io]


# ---- inputs and the oracle ------------------------------------------------------------------------------------------------------

def _torch_dtype(io):
    import torch
    return {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[io]


def _rounded(a, io):
    """float32 array -> the float32 values its storage format holds"""
    import torch
    return a if io == "f32" else torch.from_numpy(a).to(_torch_dtype(io)).float().numpy()


def _inputs_key(row):
    return (row.shape[1:], row.k, row.m, row.io, row.corner, row.outlier)


def _seed(row):
    N, S, F, G, H, W = row.shape
    return 11 + (S * 17 + F * 13 + G * 7 + H + row.k) % 9973


_BASE, _ORACLE = {}, {}


def base_inputs(row):
    """x [P, S, H, W], dy [P, F, H, W] (as stored), w, mu1, mu2 -- shared by the rows of one shape, format and offset pattern"""
    key = _inputs_key(row)
    if key not in _BASE:
        N, S, F, G, H, W = row.shape
        x, dy, w, mu1, mu2 = util.make_inputs(_seed(row), P, S, F, G, H, W, row.k, row.m)
        if row.corner is not None:
            c = row.corner
            mu1.flat[0] = c; mu2.flat[0] = -c; mu1.flat[1] = -c; mu2.flat[1] = c
        if row.outlier:
            mu1.flat[5] = 3.5
        _BASE[key] = (_rounded(x, row.io), _rounded(dy, row.io), w, mu1, mu2)
    return _BASE[key]


def group_dy(row, g):
    """the dy of image group g in the parameter-gradient call (as stored): its own, seeded by g"""
    N, S, F, G, H, W = row.shape
    rs = np.random.RandomState(100003 + g)
    return _rounded(rs.randn(P, F, H, W).astype(np.float32), row.io)


def oracle_y(row):
    from oracle import dau_oracle as orc
    key = (_inputs_key(row), "y")
    if key not in _ORACLE:
        x, dy, w, mu1, mu2 = base_inputs(row)
        _ORACLE[key] = orc.forward(x, w, mu1, mu2, 0.5)
    return _ORACLE[key]


def oracle_backward(row, g=None):
    """g None: the tiled call's dx [P, S, H, W]; else {dx, dw, dmu1, dmu2, dsigma} of image group g with group_dy(row, g)"""
    from oracle import dau_oracle as orc
    key = (_inputs_key(row), "bwd", g)
    if key not in _ORACLE:
        x, dy, w, mu1, mu2 = base_inputs(row)
        if g is None:
            _ORACLE[key] = orc.backward(x, dy, w, mu1, mu2, 0.5, need=("dx",))["dx"]
        else:
            _ORACLE[key] = orc.backward(x, group_dy(row, g), w, mu1, mu2, 0.5)
    return _ORACLE[key]


# ---- the chunked comparers (device of their arguments) ---------------------------------------------------------------------------

Parity = namedtuple("Parity", "violation nans first gotv wantv")     # first: (n, c, y, x) of the first element over the bar or NaN


def parity_chunked(got, want, rel=1e-4, floor=1e-6, chunk_elems=1 << 24):
    """util.parity_error restated in torch, for a tensor too large for the host: got [N, C, H, W] (any strides, any float dtype) holds
    want [Pw, C, H, W] (float64) tiled over N, got[n] ~ want[n % Pw].  The same float64 operations in the same order, so `violation`
    is parity_error's value to the last bit (<= 0 means pass); NaNs are counted apart and left out of the maximum.  Runs over chunks of
    whole image groups with float64 temporaries of at most chunk_elems elements (one group where a group is larger)."""
    import torch
    Pw = want.shape[0]
    N = got.shape[0]
    assert N % Pw == 0 and tuple(got.shape[1:]) == tuple(want.shape[1:]) and want.dtype == torch.float64, (got.shape, want.shape)
    scale = want.abs().max()
    tol = rel * want.abs() + floor * scale + 1e-12
    step = max(1, chunk_elems // want.numel())
    ninf = float("-inf")

    def excess(g0):
        g1 = min(g0 + step, N // Pw)
        d = got[g0 * Pw:g1 * Pw].reshape((g1 - g0, Pw) + tuple(want.shape[1:])).to(torch.float64)
        d -= want
        d.abs_()
        d -= tol
        return d

    worst = torch.full((), ninf, dtype=torch.float64, device=got.device)
    nans = torch.zeros((), dtype=torch.int64, device=got.device)
    starts = list(range(0, N // Pw, step))
    bad = []
    for g0 in starts:
        d = excess(g0)
        nan = torch.isnan(d)
        nans += nan.sum()
        top = torch.where(nan, torch.full_like(d, ninf), d).max()
        worst = torch.maximum(worst, top)
        bad.append((top > 0) | nan.any())
        del d, nan
    bad = torch.stack(bad).cpu().numpy()
    first = gotv = wantv = None
    if bad.any():
        g0 = starts[int(np.argmax(bad))]
        d = excess(g0)
        flat = int(torch.nonzero(~(d <= 0).reshape(-1))[0])
        idx = np.unravel_index(flat, tuple(d.shape))
        first = (int((g0 + idx[0]) * Pw + idx[1]),) + tuple(int(i) for i in idx[2:])
        gotv, wantv = float(got[first]), float(want[(first[0] % Pw,) + first[1:]])
    return Parity(float(worst), int(nans), first, gotv, wantv)


def _groups(mem, group_elems):
    """a contiguous activation array -> its [groups, P images' elements] matrix"""
    assert mem.is_contiguous() and mem.numel() % group_elems == 0
    return mem.reshape(-1, group_elems)


def _ints(mem):
    import torch
    return mem.view({2: torch.int16, 4: torch.int32}[mem.element_size()])


def first_group_differing(mem, group_elems, chunk_elems=1 << 26):
    """mem: a contiguous activation array in memory order, whole image groups of group_elems elements each.  -> None if every
    group has the bits of group 0, else (group, element within the group) of the first difference"""
    import torch
    m = _groups(_ints(mem), group_elems)
    step = max(1, chunk_elems // group_elems)
    flags = [(m[g0:g0 + step] != m[0:1]).any(1) for g0 in range(0, m.shape[0], step)]
    flags = torch.cat(flags).cpu().numpy()
    if not flags.any():
        return None
    g = int(np.argmax(flags))
    return g, int(torch.nonzero(m[g] != m[0])[0])


def first_group_nonzero(mem, group_elems, outside, chunk_elems=1 << 26):
    """-> None if every group but those of `outside` (which may hold anything) is zero in every element (a NaN is not zero), else
    (group, element within it) of the first one that is not"""
    import torch
    m = _groups(mem, group_elems)
    step = max(1, chunk_elems // group_elems)
    flags = torch.cat([(m[g0:g0 + step] != 0).any(1) for g0 in range(0, m.shape[0], step)]).cpu().numpy()
    flags[list(outside)] = False
    if not flags.any():
        return None
    g = int(np.argmax(flags))
    return g, int(torch.nonzero(m[g] != 0)[0])


def _locate(row, channels, g, pos):
    """(group, element within the group, in memory order) -> 'image n, byte offset b'"""
    N, S, F, G, H, W = row.shape
    n = g * P + pos // (channels * H * W)
    return "image %d, byte offset %d" % (n, (g * P * channels * H * W + pos) * ESIZE[row.io])


def assert_tensor(got_mem, want, row, channels, name, grads=False, bits=True, groups=None):
    """The whole-tensor check: got_mem, the array as the library wrote it ([N, C, H, W], or [N, H, W, C] for an NHWC row), against
    want [Pw, C, H, W] tiled over the batch at the row's bar; no NaN; and (bits) every image group bit-identical to the first."""
    import torch
    N, S, F, G, H, W = row.shape
    rel, floor = bar(row, grads)
    logical = got_mem.permute(0, 3, 1, 2) if is_nhwc(row) else got_mem
    wt = torch.from_numpy(np.asarray(want, np.float64)).to(got_mem.device)
    res = parity_chunked(logical, wt, rel, floor)
    if res.nans or res.violation > 0:
        n, c, y, x = res.first
        base = 0 if groups is None else groups * P
        limits = limits_crossed(N * channels * H * W, ESIZE[row.io])
        raise AssertionError("%s %s: %d NaN, parity violated by %.3e; first at image %d (c %d, y %d, x %d), byte offset %d: got %.7g "
                             "want %.7g; the tensor crosses %s" % (row.id, name, res.nans, res.violation, base + n, c, y, x,
                                                                  byte_offset(base + n, c, y, x, row, channels), res.gotv, res.wantv,
                                                                  [l for l, _ in limits] or "no limit"))
    if bits:
        diff = first_group_differing(got_mem, P * channels * H * W)
        assert diff is None, "%s %s: image n does not have the bits of image n %% %d: first at %s" % (
            row.id, name, P, _locate(row, channels, *diff))
    return res


# ---- the calls ------------------------------------------------------------------------------------------------------------------

def create_plan(capi, row):
    """the row's plan, created under the row's workspace budget (the default one where the row names none)"""
    N, S, F, G, H, W = row.shape
    old = os.environ.get(BUDGET)
    try:
        if row.budget is not None:
            os.environ[BUDGET] = row.budget
        elif old is not None:
            del os.environ[BUDGET]
        return capi.Plan(N, S, F, G, H, W, max_kernel_size=row.k, sigma_hint=0.5, flags=plan_flags(row), algo=row.algo)
    finally:
        if old is None:
            os.environ.pop(BUDGET, None)
        else:
            os.environ[BUDGET] = old


def memory_needed(capi, row, plan):
    """bytes a row holds at its peak: the four activation tensors, the larger workspace, and 3 GiB for the comparers' temporaries"""
    N = row.shape[0]
    px, py = per_image(row)
    ws = max(plan.workspace_bytes(capi.PASS_FORWARD), plan.workspace_bytes(capi.PASS_BACKWARD))
    return 2 * N * (px + py) * ESIZE[row.io] + ws + (3 << 30)


def _poison(t):
    import torch
    t.view(torch.uint8).fill_(0xFF)
    return t


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _tiled(base, row):
    """[P, C, H, W] float32 numpy -> the [N, ...] device array in the row's layout and storage, base tiled over the batch"""
    import torch
    t = torch.from_numpy(base).to(_torch_dtype(row.io)).to(DEVICE)
    if is_nhwc(row):
        t = t.permute(0, 2, 3, 1).contiguous()
    return t.repeat(row.shape[0] // P, 1, 1, 1)


class _Calls(object):
    """forward / backward of one plan through the C ABI, each with a poisoned workspace of exactly the pass's size"""

    def __init__(self, capi, row, plan, params):
        import torch
        self.capi, self.row, self.plan = capi, row, plan
        self.w, self.mu1, self.mu2 = (torch.from_numpy(a).to(DEVICE) for a in params)
        self.sigma = torch.full(tuple(self.w.shape), 0.5, device=DEVICE)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.ws = None
        self.ws_bytes = {}

    def _workspace(self, which, keep):
        import torch
        n = self.plan.workspace_bytes(which)
        self.ws_bytes[which] = n
        if not (keep and self.ws is not None and self.ws.numel() == n):
            self.ws = None
            self.ws = _poison(torch.empty(n, dtype=torch.uint8, device=DEVICE))
        return self.ws

    def _status(self, rc, what):
        capi = self.capi
        assert rc == capi.DAU_OK, "%s %s: %s" % (self.row.id, what, capi.lib.dau_conv_last_error())
        mx = ctypes.c_float()
        rc = capi.lib.dau_conv_check_status(self.plan._h, self.stream, _ptr(self.ws), ctypes.byref(mx))
        assert rc == capi.DAU_OK, "%s %s: status %s" % (self.row.id, what, capi.lib.dau_conv_last_error())

    def forward(self, x, y, keep=False):
        ws = self._workspace(self.capi.PASS_FORWARD, keep)
        rc = self.capi.lib.dau_conv_forward(self.plan._h, self.stream, _ptr(x), _ptr(self.w), _ptr(self.mu1), _ptr(self.mu2),
                                            _ptr(self.sigma), _ptr(y), _ptr(ws), ws.numel())
        self._status(rc, "forward")

    def outlier_status(self):
        units, taken = ctypes.c_int32(), ctypes.c_int32()
        rc = self.capi.lib.dau_conv_gather_outlier_status(self.plan._h, self.stream, _ptr(self.ws), ctypes.byref(units), ctypes.byref(taken))
        assert rc == self.capi.DAU_OK
        return units.value, bool(taken.value)

    def backward(self, x, dy, dx, grads, need, keep=False):
        ws = self._workspace(self.capi.PASS_BACKWARD, keep)
        rc = self.capi.lib.dau_conv_backward(self.plan._h, self.stream, _ptr(x), _ptr(dy), _ptr(self.w), _ptr(self.mu1), _ptr(self.mu2),
                                             _ptr(self.sigma), _ptr(dx), *([_ptr(g) for g in grads] + [_ptr(ws), ws.numel(), int(need)]))
        self._status(rc, "backward")

    def release(self):
        self.ws = None


GRADS = ("dw", "dmu1", "dmu2", "dsigma")
_FIRST = {}               # (inputs key, N, flags, algo, budget) -> the first image group's outputs, logical NCHW bits


def _first_key(row):
    return (_inputs_key(row), row.shape[0], row.flags, row.algo, row.budget)


def _first_bits(mem, row):
    head = mem[:P].permute(0, 3, 1, 2) if is_nhwc(row) else mem[:P]
    return _ints(head.contiguous()).cpu().numpy()


def run_row(capi, row, bits=True):
    """Everything the module's docstring lists, for one row.  -> a dict of what the row did (plan numbers, limits, K, wall times,
    the measured violations), also printed as one JSON line."""
    import torch
    assert DEVICE == "cuda"
    t_start = time.time()
    assert_phase(row)
    N, S, F, G, H, W = row.shape
    px, py = per_image(row)
    plan = create_plan(capi, row)
    info = plan.info
    K = key_groups(row, info["batch_slab_gather"], info["batch_slab_dot"])
    xb, dyb, w, mu1, mu2 = base_inputs(row)
    want_y, want_dx = oracle_y(row), oracle_backward(row)
    want_groups = {g: oracle_backward(row, g) for g in K}
    t_oracle = time.time() - t_start
    calls = _Calls(capi, row, plan, (w, mu1, mu2))
    rec = OrderedDict(row=row.id, shape=list(row.shape), k=row.k, io=row.io, flags=plan_flags(row), limits={k: [n for n, _ in v] for k, v in row_limits(row).items()},
                      batch_slab_gather=info["batch_slab_gather"], batch_slab_dot=info["batch_slab_dot"],
                      gather_dense_split=info["gather_dense_split"], offset_bucket=info["offset_bucket"],
                      gather_windows=info["gather_windows"], dot_windows=info["dot_windows"], algo_forward=info["algo_forward"], algo_backward=info["algo_backward"],
                      workspace_fwd=plan.workspace_bytes(capi.PASS_FORWARD), workspace_bwd=plan.workspace_bytes(capi.PASS_BACKWARD), K=K)
    first = {}
    try:
        x = _tiled(xb, row)
        y = _poison(torch.empty((N, H, W, F) if is_nhwc(row) else (N, F, H, W), dtype=x.dtype, device=DEVICE))
        t0 = time.time()
        for call in range(row.calls):
            calls.forward(x, y, keep=call > 0)            # a second call finds the first call's y and workspace
        torch.cuda.synchronize()
        rec["forward_s"] = round((time.time() - t0) / row.calls, 3)
        if row.outlier:
            assert calls.outlier_status() == (1, True), "%s: the radius-3 + ring member did not run" % row.id
        calls.release()
        res = assert_tensor(y, want_y, row, F, "y", bits=bits)
        rec["y_violation"] = res.violation
        first["y"] = _first_bits(y, row)
        del y

        dy = _tiled(dyb, row)
        dx = _poison(torch.empty_like(x))
        grads = [_poison(torch.empty(w.shape, dtype=torch.float32, device=DEVICE)) for _ in GRADS]
        t0 = time.time()
        for call in range(row.calls):
            calls.backward(x, dy, dx, [None] * 4, capi.NEED_DX, keep=call > 0)
        torch.cuda.synchronize()
        rec["backward_dx_s"] = round((time.time() - t0) / row.calls, 3)
        res = assert_tensor(dx, want_dx, row, S, "dx", bits=bits)
        rec["dx_violation"] = res.violation
        first["dx"] = _first_bits(dx, row)

        # the parameter-gradient call: dy zero but on K
        dy.zero_()
        for g in K:
            dy[g * P:(g + 1) * P] = _tiled_group(group_dy(row, g), row)
        _poison(dx)
        t0 = time.time()
        for call in range(row.calls):
            calls.backward(x, dy, dx, grads, capi.NEED_ALL, keep=call > 0)
        torch.cuda.synchronize()
        rec["backward_all_s"] = round((time.time() - t0) / row.calls, 3)
        calls.release()
        got, want = {}, {}
        rel, floor = bar(row, grads=True)
        for t, key in zip(grads, GRADS):
            got[key] = t.cpu().numpy()
            want[key] = sum(np.asarray(want_groups[g][key], np.float64) for g in K)
            first[key] = got[key].view(np.uint32).copy()
        for key in GRADS:
            util.assert_parity(got[key], want[key], "%s %s (dy on the image groups %s)" % (row.id, key, K), rel=rel, floor=floor)
        nz = first_group_nonzero(dx, P * px, K)
        assert nz is None, "%s: dx of an image whose dy is zero is not zero: %s" % (row.id, _locate(row, S, *nz))
        for g in K:
            assert_tensor(dx[g * P:(g + 1) * P], want_groups[g]["dx"], row, S, "dx of image group %d" % g, bits=False, groups=g)
        # the distances on record: y and dx of the first image group (with the bit check: of every group), the parameter gradients
        got.update(y=_widen(first["y"], row), dx=_widen(first["dx"], row))
        want.update(y=want_y, dx=want_dx)
        rec["margins"] = util.record_margins("large_batch/" + row.id, got, want, "y, dx: %g rel + %g max-norm; parameter gradients: %g + %g" % (
            bar(row) + bar(row, True)))
    finally:
        calls.release()
        x = y = dy = dx = grads = None
        torch.cuda.empty_cache()
    rec["oracle_s"] = round(t_oracle, 2)
    rec["wall_s"] = round(time.time() - t_start, 2)
    _FIRST[_first_key(row)] = first
    print(json.dumps(rec))
    return rec


def _tiled_group(base, row):
    import torch
    t = torch.from_numpy(base).to(_torch_dtype(row.io)).to(DEVICE)
    return t.permute(0, 2, 3, 1).contiguous() if is_nhwc(row) else t


def _widen(bits, row):
    import torch
    return torch.from_numpy(bits).view(_torch_dtype(row.io)).float().numpy()


def first_group(capi, row):
    """the first image group's outputs of a row as bits in logical NCHW order (running the row if it has not run in this session)"""
    if _first_key(row) not in _FIRST:
        run_row(capi, row)
    return _FIRST[_first_key(row)]
