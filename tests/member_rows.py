"""The plan-level fixtures of the feature suites (test_gpu_nhwc.py, test_gpu_epilogue.py, test_gpu_residual.py, test_gpu_input_relu.py):
the smallest shapes that reach every member, their seeded tensors, and plans that prove through Plan.info that the intended member is
held.  A suite parametrises over its tuple of row names, so a row added here joins a suite only where that suite's tuple names it.
tests/test_member_rows.py pins the generated tensors and the tuples on the CPU."""
import numpy as np
import torch

from util import make_inputs

I, UT, SD = 1 << 0, 1 << 1, 1 << 2          # USE_INTERPOLATION, UNIT_TESTING, SINGLE_DIM_KERNEL
SPLIT, NO_SPLIT, OUTLIERS = 1 << 9, 1 << 10, 1 << 12
IO = {"f32": (0, torch.float32), "f16": (1 << 11, torch.float16), "bf16": (1 << 4, torch.bfloat16)}

# name -> (flags, (N, S, F, G, H, W), k, m)
ROWS = {
    # the three radii.  S = 7 is no multiple of 8 nor of 4 and F = 5 pads: channel clamps, guarded loads of bias and residual, element
    # access in both layouts; two bands plus a short last row block; W % 4 != 0
    "split_17x13_m2": (SPLIT, (2, 7, 5, 2, 17, 13), 9, 2.0),
    "split_17x13_m3": (SPLIT, (2, 7, 5, 2, 17, 13), 9, 3.0),
    "split_17x13_m4": (SPLIT, (2, 7, 5, 2, 17, 13), 9, 3.99),
    # two 64-column segments, halo across the seam
    "split_9x70_m2": (SPLIT, (2, 7, 5, 2, 9, 70), 9, 2.0),
    "split_9x70_m3": (SPLIT, (2, 7, 5, 2, 9, 70), 9, 3.0),
    "split_9x70_m4": (SPLIT, (2, 7, 5, 2, 9, 70), 9, 3.99),
    # tall tiles, two 32-channel wave groups, 16-byte NHWC loads and stores
    "split_tall_28x28": (SPLIT, (2, 16, 40, 4, 28, 28), 9, 3.0),
    # the ring and the ADD epilogue (one unit at 3.5): planar partial sums of the ring pass; bias and residual join after the ring's sum
    "outliers_28x28": (SPLIT | OUTLIERS, (2, 16, 40, 4, 28, 28), 9, 3.0),
    "exact_stacked_28x28": (NO_SPLIT, (4, 8, 16, 6, 28, 28), 9, 3.0),     # the exact gather and gather-dot, stacked planes
    "exact_bucket8": (NO_SPLIT, (2, 5, 8, 2, 40, 72), 17, 7.0),
    "k65_33x20": (0, (2, 3, 8, 3, 33, 20), 65, 20.0),                    # gather-dot offset windows
    # four gather-sum window passes, the accumulate re-read: epilogue and input mask belong to the last
    "k65_gather_windows": (0, (2, 2, 20, 9, 37, 100), 65, 20.0),
    "unit_testing_24x24": (UT, (2, 8, 16, 4, 24, 24), 9, 3.0),
    "unit_testing_32x32": (UT, (2, 8, 16, 4, 32, 32), 9, 3.0),           # last row and column of the error dropped
    "single_dim": (SD, (2, 8, 16, 2, 16, 16), 9, 3.0),
    # the default plan: split gather radii with the chunk-pair loop, and the two-limb gather-dot
    "default_128": (0, (2, 128, 128, 4, 16, 16), 9, 3.0),
    # the tall-tile row with four images: a slab is an even number of images that divides the batch (image pairs stay together), so a
    # batch of two cannot run in slabs
    "split_tall_28x28_n4": (SPLIT, (4, 16, 40, 4, 28, 28), 9, 3.0),
}
# what each suite parametrises over, in its order
FUSED_ROWS = ("split_17x13_m2", "split_17x13_m3", "split_17x13_m4", "split_tall_28x28", "outliers_28x28", "exact_stacked_28x28",
              "exact_bucket8", "k65_gather_windows", "default_128")           # epilogue, residual, input_relu
NHWC_ROWS = ("split_17x13_m2", "split_17x13_m3", "split_17x13_m4", "split_9x70_m2", "split_9x70_m3", "split_9x70_m4", "split_tall_28x28",
             "outliers_28x28", "exact_stacked_28x28", "exact_bucket8", "k65_33x20", "k65_gather_windows", "unit_testing_24x24",
             "unit_testing_32x32", "single_dim", "default_128")
# the slab tests: test id -> the row of four images it runs
SLAB_ROWS = {"exact_stacked_28x28": "exact_stacked_28x28", "split_tall_28x28": "split_tall_28x28_n4"}


def inputs(name, x="rand"):
    """x, dy, w, mu1, mu2 of the row as float32 numpy arrays, seeded by its name; x="randn" is another, equally pinned data set whose x
    is sign-symmetric (an input ReLU cuts about half of it)"""
    flags, shape, k, m = ROWS[name]
    data = make_inputs(1 + sum(ord(c) for c in name), *shape, k, m, x=x)
    if flags & OUTLIERS:
        data[3].flat[5] = 3.5
    if flags & SD:
        data[4][:] = 0.0
    return data


def plan(name, io, nhwc=False, extra=0):
    """a fresh plan of the row with `extra` flags, after the proof that it holds the member the row is named for"""
    from dau_conv import _capi
    flags, (N, S, F, G, H, W), k, m = ROWS[name]
    p = _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5,
                   flags=I | flags | IO[io][0] | extra | (_capi.FLAG_IO_NHWC if nhwc else 0))
    if name == "default_128":
        assert p.info["gather_dense_split"] == 0b11100 and p.info["algo_backward"] == _capi.ALGO_TILED
    if name.startswith("split"):
        assert p.info["gather_dense_split"] & 0b11100 == 0b11100
    if name.startswith("exact"):
        assert p.info["gather_dense_split"] == 0
    if name == "exact_bucket8":
        assert p.info["offset_bucket"] == 8
    if name == "k65_gather_windows":
        assert p.info["gather_windows"] == 4
    if name == "unit_testing_32x32":
        assert p.info["drop_last_col"] == 1 and p.info["drop_last_row"] == 1
    if flags & OUTLIERS:
        assert p.info["gather_dense_split"] & (1 << 5)
    return p


def params(name, x="rand"):
    """w, mu1, mu2 of inputs(name, x) and a sigma of 0.5, on the device"""
    w, mu1, mu2 = (torch.from_numpy(a).cuda() for a in inputs(name, x)[2:])
    return w, mu1, mu2, torch.full(w.shape, 0.5, device="cuda")


def lay(a, plan):
    """the tensor in the plan's layout"""
    return a.contiguous(memory_format=torch.channels_last if plan.io_layout == "NHWC" else torch.contiguous_format)


def act(a, dtype, plan):
    return lay(a.to(dtype), plan)


def io_of(plan):
    return {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}[plan.io_dtype]


def nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def nhwc_view(buf, shape, offset):
    """a channels_last tensor of logical `shape` whose memory is buf[offset : offset + numel]"""
    N, C, H, W = shape
    return buf[offset:offset + N * C * H * W].view(N, H, W, C).permute(0, 3, 1, 2)
