"""GPU: the A operand of the two-limb f16 gather-dot (k_split_dot.hip) is loaded once per PAIR of K steps; the odd step's
fragment comes from the quad neighbour's registers (select + quad-permute DPP move).  The fragments that reach the MFMAs, and
their order, are those of one load per K step, so the four parameter gradients must be BIT-IDENTICAL to the build that keeps
the per-step loads (libdau_conv_hip_step_loads.so of `make tuning`: -DDAU_SD_STEP_LOADS), here on a ragged shape (nothing a
multiple of its block size; region width 12) and on one whose width takes the region width 10 (an odd number of pairs per
item).  The shipped kernel is byte-identical in the tuning build (test_built_code.py), which is the one compared.
(The x-side staging itself is unchanged: the one-pass form was measured and not kept)"""
import numpy as np
import pytest

from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, region_width, tuning_capi, variant_capi

pytestmark = pytest.mark.gpu

PARAMS = ("dw", "dmu1", "dmu2", "dsigma")


def _gradients(capi, x, dy, w, mu1, mu2):
    import torch
    N, S, H, W = x.shape
    G, F = w.shape[2:]
    plan = capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5,
                     flags=capi.FLAG_USE_INTERPOLATION | capi.FLAG_DENSE_SPLIT_F16)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
    need = capi.NEED_DW | capi.NEED_DMU1 | capi.NEED_DMU2 | capi.NEED_DSIGMA
    g = plan.backward(dev(x), dev(dy), dev(w), dev(mu1), dev(mu2), sg, need_mask=need)
    plan.check_status()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(("dx",) + PARAMS, g) if k in PARAMS}


@pytest.mark.parametrize("name,shape,rw", [("ragged", (5, 20, 24, 3, 13, 22), 12), ("width-10", (9, 16, 32, 2, 11, 27), 10)])
def test_pair_loads_are_bit_identical_to_per_step_loads(name, shape, rw):
    N, S, F, G, H, W = shape
    assert region_width(W) == rw
    x, dy, w, mu1, mu2 = make_inputs(701 + rw, N, S, F, G, H, W, 9, 3.0)
    mu1.flat[0] = 3.0; mu2.flat[0] = -3.0; mu1.flat[1] = -3.0; mu2.flat[1] = 3.0
    pair = _gradients(tuning_capi(), x, dy, w, mu1, mu2)
    step = _gradients(variant_capi("step_loads"), x, dy, w, mu1, mu2)
    want = orc.backward(x, dy, w, mu1, mu2, 0.5, need=PARAMS)
    for key in PARAMS:
        differ = int((pair[key].view(np.uint32) != step[key].view(np.uint32)).sum())
        print("%s/%s: %d of %d values differ from the per-step loads" % (name, key, differ, pair[key].size))
        assert differ == 0, "%s/%s: %d values differ" % (name, key, differ)
        assert_parity(step[key], want[key], name + "/" + key)      # the reference itself is right
